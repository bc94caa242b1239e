r"""Doubles the frame rate of a YUV4MPEG2 (.y4m) video: n frames in, 2 n - 1 frames out - every input frame verbatim, with the
mid-frame of each consecutive pair between them.  Video in, video out: the frames stay 8-bit Y'CbCr 4:2:0 from the file to the GPU and
back (a frame stream with pix 'i420': the colour conversion runs inside the engine's tile cut and quantisation, one feature extraction
per frame), no PNGs, no ffmpeg, a few frames of memory.

  cd frame-interpolation_amd
  python -m eval.video_cli --model_path <model dir> --input in.y4m --output out.y4m
  ffmpeg -i a.mp4 -f yuv4mpegpipe - | python -m eval.video_cli --model_path <model dir> --input - --output - | ffmpeg -i - b.mp4

The output header keeps the input's tokens with the frame rate (F) doubled.  What is read: film_hip/y4m.py (8-bit 4:2:0, progressive).
"""
import argparse
import sys
from typing import Optional

from film_hip import y4m

from . import interpolator as interpolator_lib


def build_parser() -> argparse.ArgumentParser:
    """Model and tiling flags as eval/interpolator_cli.py."""
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--input', required=True, help='The .y4m file to read, or - for stdin.')
    ap.add_argument('--output', required=True, help='The .y4m file to write, or - for stdout.')
    ap.add_argument('--model_path', default=None, help='The path of the saved model to use.')
    ap.add_argument('--align', type=int, default=64, help='If >1, pad the input size so it is evenly divisible by this value.')
    ap.add_argument('--block_height', type=int, default=1, help='Number of patches along height.')
    ap.add_argument('--block_width', type=int, default=1, help='Number of patches along width.')
    ap.add_argument('--block_overlap_height', type=int, default=0,
                    help='Rows every patch takes from its neighbours (cross-faded); 0: disjoint patches; -1: what the align padding holds.')
    ap.add_argument('--block_overlap_width', type=int, default=0, help='The same for columns.')
    ap.add_argument('--matrix', choices=['bt709', 'bt601'], default='bt709', help="The Y'CbCr matrix of the video.")
    ap.add_argument('--full_range', action='store_true', default=None,
                    help='Full-range samples (0..255); default: what the header says (XCOLORRANGE=FULL), else limited range.')
    return ap


def double_frame_rate(it, reader: y4m.Y4MReader, out, matrix: str = 'bt709', full_range: Optional[bool] = None) -> int:
    """Streams reader's frames through an I420 stream of `it` (an eval.interpolator.Interpolator) and writes the doubled video to the
    binary file object `out`.  Returns the number of frames written.  One input frame and one mid-frame are alive at a time."""
    full = reader.full_range if full_range is None else bool(full_range)
    writer = y4m.Y4MWriter(out, y4m.double_rate(reader.tokens))
    with it.open_stream(reader.height, reader.width, pix='i420', matrix=matrix, full_range=full) as st:
        for frame in reader:
            mid = st.push(frame)
            if mid is not None:
                writer.write(mid)
            writer.write(frame)
    return writer.frames_written


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)
    fin = sys.stdin.buffer if args.input == '-' else open(args.input, 'rb')
    try:
        reader = y4m.Y4MReader(fin)       # (the header's refusals come before the model is loaded)
        overlap = (args.block_overlap_height, args.block_overlap_width)
        it = interpolator_lib.Interpolator(args.model_path, args.align, [args.block_height, args.block_width],
                                           **({'block_overlap': overlap} if any(overlap) else {}))
        fout = sys.stdout.buffer if args.output == '-' else open(args.output, 'wb')
        try:
            n = double_frame_rate(it, reader, fout, args.matrix, args.full_range)
            fout.flush()
        finally:
            if fout is not sys.stdout.buffer:
                fout.close()
    finally:
        if fin is not sys.stdin.buffer:
            fin.close()
    print(f'{args.input}: {reader.frames_read} frames in, {n} frames out', file=sys.stderr)
    return n


if __name__ == '__main__':
    main()
