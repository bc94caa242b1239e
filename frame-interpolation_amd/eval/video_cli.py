r"""Doubles the frame rate of a YUV4MPEG2 (.y4m) video: n frames in, 2 n - 1 frames out - every input frame verbatim, with the
mid-frame of each consecutive pair between them.  --times_to_interpolate T multiplies it by 2^T instead: (n - 1) 2^T + 1 frames, the
2^T - 1 frames of the reference's recursion between every two input frames (one push of a "stream_times" = T stream: the mid-frames
that are interpolated further stay float32 on the GPU, only the output is quantised, and every frame is extracted once).  Video in, video out: the frames stay 8-bit Y'CbCr 4:2:0 from the file to the GPU and
back (a frame stream with pix 'i420': the colour conversion runs inside the engine's tile cut and quantisation, one feature extraction
per frame), no PNGs, no ffmpeg, a few frames of memory.  A 10-bit stream (C420p10, `ffmpeg -pix_fmt yuv420p10le`) stays 10-bit the same
way (pix 'i010'): no flag is needed, the header says it.

  cd frame-interpolation_amd
  python -m eval.video_cli --model_path <model dir> --input in.y4m --output out.y4m
  ffmpeg -i a.mp4 -f yuv4mpegpipe - | python -m eval.video_cli --model_path <model dir> --input - --output - | ffmpeg -i - b.mp4

--scene_cut PERMILLE (default 0: off) lets the engine look for scene cuts (film_set_option "scene_cut", include/film_hip.h: the distance
of consecutive frames' sample histograms, in permille of its maximum): across a cut no mid-frame is generated and the frame before the
cut is written again in their place (a frame hold: once, or 2^T - 1 times), so the output keeps its frame count at a uniform rate.  No value is recommended:
the detector's hit and miss rates on real footage are unmeasured.

The output header keeps the input's tokens with the frame rate (F) doubled (multiplied by 2^T).  What is read: film_hip/y4m.py (8-bit and 10-bit 4:2:0, progressive).
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
                    help='Full-range samples (0..255, 10-bit: 0..1023); default: what the header says (XCOLORRANGE=FULL), else limited range.')
    ap.add_argument('--scene_cut', type=int, default=0, metavar='PERMILLE',
                    help='Treat a pair of frames whose histogram distance reaches this many permille (1..1000) as a scene cut: the frame '
                         'before the cut is held instead of a mid-frame.  0 (default): off.  No value is recommended (unmeasured on footage).')
    ap.add_argument('--times_to_interpolate', type=int, default=1, metavar='T',
                    help='1 .. 6: multiply the frame rate by 2^T - 2^T - 1 frames between every two input frames, the recursion of the '
                         'reference.  1 (default): double it.')
    return ap


def double_frame_rate(it, reader: y4m.Y4MReader, out, matrix: str = 'bt709', full_range: Optional[bool] = None, scene_cut: int = 0,
                      cuts: Optional[list] = None, times: int = 1) -> int:
    """Streams reader's frames through an I420 stream (I010 for a 10-bit reader) of `it` (an eval.interpolator.Interpolator) and writes the doubled video to the
    binary file object `out`.  Returns the number of frames written.  One input frame and one mid-frame are alive at a time (two input
    frames with scene_cut).  scene_cut > 0 (permille, engine option "scene_cut"): a push after the first that returns no mid-frame is
    a scene cut - the previous input frame is written again in the mid-frame's place; `cuts` (a list) receives the index of every input
    frame that starts a new scene.
    times = T > 1: the frame rate times 2^T - a push returns the 2^T - 1 frames between two input frames (a stream opened with times=T),
    and the hold across a cut writes the previous frame that many times."""
    times = int(times)
    if not 1 <= times <= 6:
        raise ValueError(f'times_to_interpolate must be 1 .. 6, got {times}')
    full = reader.full_range if full_range is None else bool(full_range)
    writer = y4m.Y4MWriter(out, y4m.multiply_rate(reader.tokens, 1 << times))
    with it.open_stream(reader.height, reader.width, pix='i010' if getattr(reader, 'depth', 8) == 10 else 'i420', matrix=matrix, full_range=full,
                        **({'scene_cut': int(scene_cut)} if scene_cut else {}), **({'times': times} if times != 1 else {})) as st:
        prev = None
        for i, frame in enumerate(reader):
            mid = st.push(frame)
            if mid is not None:
                for m in (mid,) if times == 1 else mid:
                    writer.write(m)
            elif scene_cut and prev is not None:
                for _ in range((1 << times) - 1):
                    writer.write(prev)      # a frame hold across the cut
                if cuts is not None:
                    cuts.append(i)
            writer.write(frame)
            prev = frame if scene_cut else None
    return writer.frames_written


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)
    if not 1 <= args.times_to_interpolate <= 6:
        raise SystemExit('--times_to_interpolate must be 1 .. 6')
    fin = sys.stdin.buffer if args.input == '-' else open(args.input, 'rb')
    try:
        reader = y4m.Y4MReader(fin, depths=(8, 10))       # (the header's refusals come before the model is loaded)
        overlap = (args.block_overlap_height, args.block_overlap_width)
        it = interpolator_lib.Interpolator(args.model_path, args.align, [args.block_height, args.block_width],
                                           **({'block_overlap': overlap} if any(overlap) else {}))
        fout = sys.stdout.buffer if args.output == '-' else open(args.output, 'wb')
        try:
            cuts = []
            n = double_frame_rate(it, reader, fout, args.matrix, args.full_range, args.scene_cut, cuts, args.times_to_interpolate)
            fout.flush()
        finally:
            if fout is not sys.stdout.buffer:
                fout.close()
    finally:
        if fin is not sys.stdin.buffer:
            fin.close()
    print(f'{args.input}: {reader.frames_read} frames in, {n} frames out' +
          (f', {len(cuts)} scene cuts' + (f' (the first at input frame {cuts[0]})' if cuts else '') if args.scene_cut else ''), file=sys.stderr)
    return n


if __name__ == '__main__':
    main()
