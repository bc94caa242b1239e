"""ctypes binding of libfilm_hip.so (C-ABI: include/film_hip.h).

This is the whole Python <-> native boundary of the product path: plain pointers and sizes.
If the shared library is missing or no MI355X is visible, construction FAILS LOUDLY - there is no
CPU or PyTorch fallback anywhere in the product path.
"""
from __future__ import annotations

import ctypes
import json
import os
from typing import Dict, Optional, Tuple

import numpy as np

from . import pixfmt
from .options import Options, PUBLISHED

_HERE = os.path.dirname(os.path.abspath(__file__))
# FILM_HIP_LIB=<path> names the library explicitly; FILM_EXTRA_FAMILIES=1 selects the flavour that also holds the opt-in kernel
# families (bf16 precision modes, F(2,3) / halo kernels: film_hip/build.py), built next to the default one
LIB_PATH = os.environ.get('FILM_HIP_LIB') or os.path.join(
    _HERE, 'libfilm_hip_extra.so' if os.environ.get('FILM_EXTRA_FAMILIES', '0') not in ('', '0') else 'libfilm_hip.so')

FILM_MEM_HOST = 0
FILM_MEM_DEVICE = 1
FILM_ERR_INVALID = -1
FILM_ERR_STATE = -2
FILM_ERR_NO_DEVICE = -3
FILM_ERR_NOMEM = -5
# pixel types of a frame stream (film_stream_open): film_hip/pixfmt.py's table under the names of include/film_hip.h, FILM_PIX_F32 ... FILM_PIX_I410
globals().update({'FILM_PIX_' + lay.name.upper(): lay.code for lay in pixfmt.LAYOUTS})
PIX = {lay.name: (lay.code, lay.dtype) for lay in pixfmt.LAYOUTS}
YUV420, YUV422, YUV444 = pixfmt.names('420'), pixfmt.names('422'), pixfmt.names('444')      # frames [H * 3 // 2, W], [2 * H, W], [3 * H, W]
YUV = YUV420 + YUV422 + YUV444
# colour flags of the Y'CbCr pixel types (added to the layout code)
FILM_YUV_BT601, FILM_YUV_FULL, FILM_YUV_BT2020 = 0x100, 0x400, 0x2000
YUV_MATRIX = {'bt709': 0, 'bt601': FILM_YUV_BT601, 'bt2020nc': FILM_YUV_BT2020}


def pix_code(pix: str, matrix: str = 'bt709', full_range: bool = False) -> int:
    """The `pix` argument of the C-ABI: the layout code of `pix` plus the colour flags (which only the Y'CbCr layouts accept)."""
    if pix not in PIX:
        raise ValueError(f'pix must be one of {sorted(PIX)}, got {pix!r}')
    if matrix not in YUV_MATRIX:
        raise ValueError(f"matrix must be 'bt709', 'bt601' or 'bt2020nc', got {matrix!r}")
    return PIX[pix][0] | YUV_MATRIX[matrix] | (FILM_YUV_FULL if full_range else 0)


frame_shape = pixfmt.frame_shape
# film_image_metrics flags (include/film_hip.h); METRIC_FLAGS maps the metric names of eval/metrics.py to them
FILM_METRIC_L1, FILM_METRIC_L2, FILM_METRIC_PSNR, FILM_METRIC_SSIM, FILM_METRIC_CLIP = 1, 2, 4, 8, 16
METRIC_FLAGS = {'l1': FILM_METRIC_L1, 'l2': FILM_METRIC_L2, 'psnr': FILM_METRIC_PSNR, 'ssim': FILM_METRIC_SSIM}
_MAXS = 8


class FilmError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f'libfilm_hip error {code}: {msg}')
        self.code = code
        self.msg = msg


class _Config(ctypes.Structure):
    _fields_ = [('pyramid_levels', ctypes.c_int32), ('fusion_pyramid_levels', ctypes.c_int32),
                ('specialized_levels', ctypes.c_int32), ('sub_levels', ctypes.c_int32),
                ('filters', ctypes.c_int32), ('flow_convs', ctypes.c_int32 * _MAXS),
                ('flow_filters', ctypes.c_int32 * _MAXS)]


# every symbol include/film_hip.h declares; tests assert the library exports all of them
EXPORTED_SYMBOLS = (
    'film_default_config', 'film_create', 'film_destroy', 'film_last_error', 'film_set_weight',
    'film_finalize', 'film_packed_size', 'film_export_packed', 'film_import_packed', 'film_export_layouts', 'film_forward',
    'film_interpolate',
    'film_set_option', 'film_profile_json', 'film_plan_json', 'film_get_tap', 'film_crc32c', 'film_version',
    'film_export_tune', 'film_import_tune', 'film_to_uint8', 'film_load_bundle', 'film_bcast_weights',
    'film_interpolate_sequence', 'film_sequence_plan_json', 'film_image_metrics', 'film_tiling_json',
    'film_debug_arena', 'film_debug_run_op', 'film_debug_tile_map',
    'film_stream_open', 'film_stream_push', 'film_stream_reset', 'film_stream_close', 'film_stream_plan_json',
    'film_to_yuv420', 'film_to_yuv', 'film_debug_yuv_cut', 'film_frame_histogram', 'film_stream_cut_info',
    'film_stream_pair_plan_json', 'film_stream_schedule_json', 'film_stream_select', 'film_stream_select_schedule_json',
    'film_frame_diff', 'film_stream_dup_info', 'film_stream_layout_json', 'film_stream_group_schedule_json', 'film_debug_segment_copy')

_lib = None


def load_library(path: Optional[str] = None) -> ctypes.CDLL:
    """dlopen()s the engine; raises if it has not been built (python __graft_entry__.py build)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.isfile(p):
        raise FileNotFoundError(
            f'{p} not found: build the HIP engine first (python -c "import __graft_entry__ as g; g.build()" '
            'or make -C frame-interpolation_amd/csrc). There is no CPU fallback.')
    if os.environ.get('FILM_NO_TORCH', '0') in ('', '0'):
        try:
            # PyTorch-ROCm bundles its own HIP runtime; importing it first makes libfilm_hip.so (whose
            # DT_NEEDED is the unversioned "libamdhip64.so", see film_hip/build.py) bind to that same
            # runtime, so device pointers and streams can be exchanged with torch.  Without torch (or with
            # FILM_NO_TORCH=1: a torch-free host, tools/graph_race_check.py on the system runtime) the
            # runtime under /opt/rocm/lib is used.
            import torch  # noqa: F401
        except Exception:  # pragma: no cover
            pass
    lib = ctypes.CDLL(p)
    vp, cp, i64p, fp = ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int64), ctypes.c_void_p
    lib.film_default_config.argtypes = [ctypes.POINTER(_Config)]
    lib.film_create.argtypes = [ctypes.POINTER(vp), ctypes.c_int, ctypes.POINTER(_Config)]
    lib.film_destroy.argtypes = [vp]
    lib.film_destroy.restype = None
    lib.film_last_error.argtypes = [vp]
    lib.film_last_error.restype = cp
    lib.film_set_weight.argtypes = [vp, cp, fp, i64p, ctypes.c_int]
    lib.film_finalize.argtypes = [vp]
    lib.film_packed_size.argtypes = [vp, i64p]
    lib.film_export_packed.argtypes = [vp, fp, ctypes.c_int64, ctypes.c_int]
    lib.film_import_packed.argtypes = [vp, fp, ctypes.c_int64, ctypes.c_int]
    lib.film_export_layouts.argtypes = [vp, fp, ctypes.c_int64, i64p]
    lib.film_forward.argtypes = [vp, fp, fp, ctypes.c_int, ctypes.c_int, ctypes.c_int, fp, ctypes.c_int, vp]
    lib.film_interpolate.argtypes = [vp, fp, fp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                     ctypes.c_int, fp, ctypes.c_int, vp]
    lib.film_interpolate_sequence.argtypes = [vp, fp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                              ctypes.c_int, fp, ctypes.c_int, vp]
    lib.film_set_option.argtypes = [vp, cp, ctypes.c_int64]
    lib.film_profile_json.argtypes = [vp, ctypes.c_char_p, ctypes.c_int64, i64p]
    lib.film_plan_json.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_int64, i64p]
    lib.film_sequence_plan_json.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_char_p,
                                            ctypes.c_int64, i64p]
    lib.film_tiling_json.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_char_p,
                                     ctypes.c_int64, i64p]
    lib.film_get_tap.argtypes = [vp, cp, fp, ctypes.c_int64, i64p]
    lib.film_crc32c.argtypes = [ctypes.c_uint32, vp, ctypes.c_int64]
    lib.film_crc32c.restype = ctypes.c_uint32
    lib.film_version.argtypes = []
    lib.film_version.restype = cp
    lib.film_export_tune.argtypes = [vp, ctypes.c_char_p, ctypes.c_int64, i64p]
    lib.film_import_tune.argtypes = [vp, cp]
    lib.film_to_uint8.argtypes = [vp, vp, ctypes.c_int64, vp]
    lib.film_load_bundle.argtypes = [vp, cp, ctypes.c_int, ctypes.c_char_p, ctypes.c_int64, i64p]
    lib.film_bcast_weights.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, vp]
    lib.film_image_metrics.argtypes = [vp, fp, fp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                       ctypes.c_double, fp, ctypes.c_int, vp]
    lib.film_debug_arena.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_int64, fp, ctypes.c_int]
    lib.film_debug_run_op.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                      ctypes.POINTER(ctypes.c_int)]
    lib.film_debug_tile_map.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                        ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp]
    lib.film_to_yuv420.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp]
    lib.film_to_yuv.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp]
    lib.film_debug_yuv_cut.argtypes = [vp, ctypes.c_int, vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                       ctypes.c_int, ctypes.c_int, ctypes.c_int, vp]
    lib.film_stream_open.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    lib.film_stream_push.argtypes = [vp, vp, vp, ctypes.POINTER(ctypes.c_int), ctypes.c_int, vp]
    lib.film_stream_reset.argtypes = [vp]
    lib.film_stream_close.argtypes = [vp]
    lib.film_stream_plan_json.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_int64, i64p]
    lib.film_frame_histogram.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, vp]
    lib.film_stream_pair_plan_json.argtypes = [vp] + [ctypes.c_int] * 7 + [ctypes.c_char_p, ctypes.c_int64, i64p]
    lib.film_stream_schedule_json.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_int64, i64p]
    lib.film_stream_select.argtypes = [vp, ctypes.c_uint64]
    lib.film_stream_select_schedule_json.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_int64, i64p]
    lib.film_stream_layout_json.argtypes = [vp, ctypes.c_char_p, ctypes.c_int64, i64p]
    lib.film_stream_group_schedule_json.argtypes = [vp] + [ctypes.c_int] * 5 + [ctypes.c_uint64, ctypes.c_int, ctypes.c_char_p, ctypes.c_int64, i64p]
    lib.film_debug_segment_copy.argtypes = [i64p, ctypes.c_int, vp, vp, vp]
    lib.film_stream_cut_info.argtypes = [vp, i64p, i64p, ctypes.POINTER(ctypes.c_int)]
    lib.film_frame_diff.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, vp]
    lib.film_stream_dup_info.argtypes = [vp, i64p, ctypes.POINTER(ctypes.c_int)]
    for name in EXPORTED_SYMBOLS:
        fn = getattr(lib, name)
        if fn.restype is ctypes.c_int and name not in ('film_destroy',):
            fn.restype = ctypes.c_int
    if path is None:
        _lib = lib
    return lib


def hip_runtime_info() -> Tuple[str, int, str]:
    """(path, hipRuntimeGetVersion(), 'major.minor.patch') of the HIP runtime libfilm_hip.so is bound to in THIS process: PyTorch's
    bundled libamdhip64.so when torch was imported first, /opt/rocm/lib's otherwise (film_hip/build.py).  HIP_VERSION is
    major * 10^7 + minor * 10^5 + patch: 70226015 is HIP 7.2.26015, not 7.0.2."""
    load_library()
    path = ''
    with open('/proc/self/maps') as f:
        for line in f:
            if 'libamdhip64' in line:
                path = line.split()[-1]
                break
    if not path:
        return '', 0, 'not loaded'
    v = ctypes.c_int(0)
    ctypes.CDLL(path).hipRuntimeGetVersion(ctypes.byref(v))
    return path, v.value, f'{v.value // 10000000}.{v.value // 100000 % 100}.{v.value % 100000}'


def _cfg_struct(opt: Options) -> _Config:
    opt.validate()
    c = _Config()
    c.pyramid_levels, c.fusion_pyramid_levels = opt.pyramid_levels, opt.fusion_pyramid_levels
    c.specialized_levels, c.sub_levels, c.filters = opt.specialized_levels, opt.sub_levels, opt.filters
    for i, (a, b) in enumerate(zip(opt.flow_convs, opt.flow_filters)):
        c.flow_convs[i] = a
        c.flow_filters[i] = b
    return c


def frame_histogram_device(ptr: int, h: int, w: int, hist_ptr: int, pix: str = 'u8', matrix: str = 'bt709', full_range: bool = False,
                           stream: Optional[int] = None) -> None:
    """film_frame_histogram: the 3 x 256 sample histogram (include/film_hip.h, "Scene cuts") of ONE h x w device frame of pixel type `pix`
    into 768 device uint32 at hist_ptr (overwritten), asynchronous on `stream` of the current device.  ptr must be 4-byte aligned and an
    8-bit frame lie in an allocation of whole 32-bit words (so must a 10-bit 4:4:4 frame of odd size).  A 10-bit sample counts in the bin of its code >> 2.
    Needs no engine."""
    rc = load_library().film_frame_histogram(ctypes.c_void_p(ptr), int(h), int(w), pix_code(pix, matrix, full_range), ctypes.c_void_p(hist_ptr),
                                             ctypes.c_void_p(stream) if stream else None)
    if rc != 0:
        raise FilmError(rc, 'film_frame_histogram failed')


def frame_diff_device(ptr_a: int, ptr_b: int, h: int, w: int, out_ptr: int, pix: str = 'u8', matrix: str = 'bt709', full_range: bool = False,
                      lo: int = 0, stream: Optional[int] = None) -> None:
    """film_frame_diff: the 8 x 8 block SAD statistics (include/film_hip.h, "Duplicate frames") of TWO h x w device frames of pixel type `pix`
    into 12 device uint64 at out_ptr ([3][4]: total, max, over, blocks per plane; overwritten), asynchronous on `stream` of the current device.
    `over` counts the blocks whose SAD is > lo (0 .. 65535, stored-code units).  The frame pointers follow frame_histogram_device's contract,
    out_ptr is 8-byte aligned.  Needs no engine."""
    rc = load_library().film_frame_diff(ctypes.c_void_p(ptr_a), ctypes.c_void_p(ptr_b), int(h), int(w), pix_code(pix, matrix, full_range), int(lo),
                                        ctypes.c_void_p(out_ptr), ctypes.c_void_p(stream) if stream else None)
    if rc != 0:
        raise FilmError(rc, 'film_frame_diff failed')


def segment_copy_device(segs, src_ptr: int, dst_ptr: int, stream: Optional[int] = None) -> None:
    """film_debug_segment_copy: ONE launch of the kernel a grouped stream moves its carry with - segs, up to 32 rows of (source float offset,
    destination float offset, count): dst[d : d + count] = src[s : s + count] on two float32 device buffers, bit for bit, asynchronous on
    `stream` of the current device.  Needs no engine."""
    table = np.ascontiguousarray(np.asarray(segs, np.int64).reshape(-1, 3))
    rc = load_library().film_debug_segment_copy(table.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), int(table.shape[0]), ctypes.c_void_p(src_ptr),
                                                ctypes.c_void_p(dst_ptr), ctypes.c_void_p(stream) if stream else None)
    if rc != 0:
        raise FilmError(rc, 'film_debug_segment_copy failed')


def dedup_options(dedup) -> Tuple[int, int, int]:
    """open_stream(dedup=...) as the options ("dup_hi", "dup_lo", "dup_frac"): hi, or (hi, lo, frac)."""
    given = tuple(dedup) if isinstance(dedup, (tuple, list)) else (dedup,)
    if not 1 <= len(given) <= 3:
        raise ValueError(f'dedup is hi or (hi, lo, frac), got {dedup!r}')
    hi, lo, frac = given + (0, 1000)[len(given) - 1:]
    return int(hi), int(lo), int(frac)


def selection_mask(times: int, positions) -> int:
    """film_stream_select's mask of 1-based positions of a "stream_times" = times push (bit i - 1: position i); None: all 2^times - 1."""
    n = (1 << int(times)) - 1
    if positions is None:
        return (1 << n) - 1
    mask = 0
    for i in positions:
        if int(i) != i or not 1 <= i <= n:
            raise ValueError(f'a position of a times = {times} push is an integer 1 .. {n}, got {i!r}')
        mask |= 1 << (int(i) - 1)
    return mask


class FilmStream:
    """One open frame stream of an engine (film_stream_*; FilmEngine.open_stream): push() one frame at a time and get the mid-frame
    between it and the frame pushed before - bit-identical to interpolate_frames(previous, frame) - with one feature extraction per
    frame.  Frames and results are [H,W,3] float32 ('f32') or uint8 ('u8': x = u8 / 255, result = eval.util.to_uint8's bytes), or
    8-bit Y'CbCr 4:2:0 frames ('i420', 'nv12') as uint8 [H * 3 // 2, W]: the Y plane, then the Cb and Cr planes (I420) or the plane of
    CbCr pairs (NV12), with `matrix` 'bt709' | 'bt601' and limited or full range (the arithmetic: include/film_hip.h); or 10-bit 4:2:0
    frames ('i010': the code in bits 0-9, = yuv420p10le; 'p010': the code in bits 6-15) as uint16 [H * 3 // 2, W] with the same planes;
    or planar 4:2:2 ('i422' uint8, 'i210' uint16; W even) as [2 * H, W] and planar 4:4:4 ('i444' uint8, 'i410' uint16; any size) as [3 * H, W].
    `matrix` may also be 'bt2020nc' (BT.2020 non-constant luminance), with every Y'CbCr layout.
    With the engine option "scene_cut" > 0 (FilmEngine.open_stream(scene_cut=...)) a push that the histogram rule calls a scene cut returns
    None / False like a first push, and cut_info() tells the two apart.
    times = T > 1 (FilmEngine.open_stream(times=...); engine option "stream_times", read when the stream opens): a primed push returns
    the 2^T - 1 frames of the reference's times_to_interpolate = T recursion between the two frames, [2^T - 1, *shape] in temporal
    order - every one bit-identical to interpolate_frames on its float32 parents, quantised (if at all) only on the way out.
    select(positions) narrows a primed push to some of those positions (a frame-rate conversion that is no power of two:
    film_hip/retime.py): only they and their ancestors in the recursion are run, and the push returns [len(selection), *shape].
    One stream per engine at a time; use it as a context manager or close() it."""

    def __init__(self, engine: 'FilmEngine', h: int, w: int, align: Optional[int], block_shape, pix: str, matrix: str = 'bt709',
                 full_range: bool = False, times: int = 1):
        self._code = pix_code(pix, matrix, full_range)
        self._eng = engine
        self.times = int(times)                  # what the engine option said when the stream was opened
        self.per_push = (1 << self.times) - 1    # frames of a primed push with every position selected
        self.selection = tuple(range(1, self.per_push + 1))   # select(): the 1-based positions a primed push returns, ascending
        self.shape = frame_shape(pix, h, w)
        self.pix = pix
        self.dtype = PIX[pix][1]
        bh, bw = (int(block_shape[0]), int(block_shape[1])) if block_shape else (1, 1)
        engine._check(engine._lib.film_stream_open(engine._h, int(h), int(w), int(align or 0), bh, bw, self._code))
        self._open = True

    def push(self, frame: np.ndarray, out: Optional[np.ndarray] = None) -> Optional[np.ndarray]:
        """frame: host array of the stream's shape and dtype.  None for the first frame after open / reset, else the mid-frame
        (a new array, or `out`: a writable C-contiguous array of the frame's shape and dtype).  None too for a frame that option
        "scene_cut" found to start a new scene (`out` is then left as it was).  times > 1: the result and `out` are
        [2^times - 1, *frame shape] - a float32 caller does well to reuse one `out`: at 1080p with times = 2 a push into the fresh
        75 MB array measured 3 ms per frame slower than into a reused one (profiles/stream_recursion_bench.log).  After select():
        [len(selection), *frame shape], and None whenever nothing was produced - an empty selection included."""
        a = np.asarray(frame)
        if a.dtype != self.dtype or a.shape != self.shape:
            raise ValueError(f'expected a {np.dtype(self.dtype).name} array of shape {self.shape}, got {a.dtype} {a.shape}')
        a = np.ascontiguousarray(a)
        oshape = self.shape if self.times == 1 else (len(self.selection),) + self.shape
        if out is None:
            out = np.empty(oshape, self.dtype)
        elif out.dtype != self.dtype or out.shape != oshape or not out.flags['C_CONTIGUOUS'] or not out.flags['WRITEABLE']:
            raise ValueError(f'out must be a writable C-contiguous {np.dtype(self.dtype).name} array of shape {oshape}')
        produced = ctypes.c_int(0)
        eng = self._eng
        eng._check(eng._lib.film_stream_push(eng._h, a.ctypes.data, out.ctypes.data, ctypes.byref(produced), FILM_MEM_HOST, None))
        eng.save_tune_cache()
        return out if produced.value else None

    def push_device(self, ptr_in: int, ptr_out: int, stream: Optional[int] = None):
        """Device-resident push: raw device pointers to one frame of the stream's pixel type (ptr_out: to 2^times - 1 of them),
        asynchronous on `stream`.  times == 1: returns whether ptr_out receives a mid-frame (False for the first frame after open /
        reset; ptr_out may then be 0 - and for a scene cut found by option "scene_cut", which leaves ptr_out untouched).
        times > 1: returns the number of frames written, 2^times - 1 (after select(): len(selection), which ptr_out holds) or 0."""
        produced = ctypes.c_int(0)
        eng = self._eng
        eng._check(eng._lib.film_stream_push(eng._h, ctypes.c_void_p(ptr_in), ctypes.c_void_p(ptr_out) if ptr_out else None,
                                             ctypes.byref(produced), FILM_MEM_DEVICE, ctypes.c_void_p(stream) if stream else None))
        return bool(produced.value) if self.times == 1 else produced.value

    def select(self, positions=None) -> None:
        """film_stream_select: from the next push on a primed push returns only the frames at `positions` - an iterable of 1-based
        positions 1 .. 2^times - 1 (duplicates count once), or None for all - in temporal order, each bit-identical to that frame of a
        full push; only they and their ancestors in the recursion are run (FilmEngine.stream_schedule(times, slot, select=...)).  The
        selection holds until it is changed; reset() and scene cuts keep it."""
        mask = selection_mask(self.times, positions)
        self._eng._check(self._eng._lib.film_stream_select(self._eng._h, mask))
        self.selection = tuple(i for i in range(1, self.per_push + 1) if mask >> (i - 1) & 1)

    def reset(self) -> None:
        """Forgets the carried frame (scene cut, seek): the next push produces nothing.  The selection stays."""
        self._eng._check(self._eng._lib.film_stream_reset(self._eng._h))

    def layout(self) -> dict:
        """film_stream_layout_json: how the open stream runs its frame - 'tiles', 'groups' (1: the whole frame in one invocation), 'group_tiles',
        'slots', 'workspace_bytes', 'carry_bytes' and, for a stream of several tile groups, the carry buffers and the segments of every
        (group, slot) state (include/film_hip.h, "Tile groups")."""
        return self._eng._json_call(self._eng._lib.film_stream_layout_json)

    def cut_info(self) -> Tuple[int, int, int]:
        """film_stream_cut_info: (distance, samples, cut) of the last push - the histogram distance D to the frame before (-1: no
        comparison was made), the samples S of one frame, and 1 if the push was treated as a scene cut."""
        d, n, c = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int(0)
        self._eng._check(self._eng._lib.film_stream_cut_info(self._eng._h, ctypes.byref(d), ctypes.byref(n), ctypes.byref(c)))
        return d.value, n.value, c.value

    def dup_info(self):
        """film_stream_dup_info: (stats, dup) of the last push - stats the int64 [3, 4] block statistics (total, max, over, blocks per plane)
        of the pushed frame against the carried one, or None when no comparison was made; dup 1 if the push was dropped as a duplicate
        (it returned None / False like a first push and changed nothing)."""
        stats, c = (ctypes.c_int64 * 12)(), ctypes.c_int(0)
        self._eng._check(self._eng._lib.film_stream_dup_info(self._eng._h, stats, ctypes.byref(c)))
        a = np.array(stats[:], np.int64).reshape(3, 4)
        return (None if (a < 0).all() else a), c.value

    def close(self) -> None:
        if self._open and getattr(self._eng, '_h', None) is not None and self._eng._h.value:
            self._open = False
            self._eng._check(self._eng._lib.film_stream_close(self._eng._h))
        self._open = False

    def __enter__(self) -> 'FilmStream':
        return self

    def __exit__(self, *exc) -> None:
        self.close()


class FilmEngine:
    """One engine = one GPU + one stream + packed weights + cached per-shape plans.

    ``device=-1`` gives a plan-only handle (no GPU needed): it can pack weights and describe plans
    but every compute call raises FilmError(FILM_ERR_NO_DEVICE)."""

    def __init__(self, opt: Options = PUBLISHED, device: int = 0):
        self._lib = load_library()
        self._opt = opt
        self._h = ctypes.c_void_p()
        cfg = _cfg_struct(opt)
        rc = self._lib.film_create(ctypes.byref(self._h), device, ctypes.byref(cfg))
        if rc != 0:
            msg = self._lib.film_last_error(None).decode('utf-8', 'replace')
            self._h = ctypes.c_void_p()
            raise FilmError(rc, msg)
        self.device = device

    # -- lifetime ---------------------------------------------------------------------------
    def close(self) -> None:
        if getattr(self, '_h', None) is not None and self._h.value:
            self._lib.film_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int) -> None:
        if rc != 0:
            raise FilmError(rc, self._lib.film_last_error(self._h).decode('utf-8', 'replace'))

    @property
    def options(self) -> Options:
        return self._opt

    # -- weights ----------------------------------------------------------------------------
    def set_weights(self, weights: Dict[str, np.ndarray]) -> None:
        """weights: canonical name -> HWIO kernel / bias (film_hip.weights)."""
        for name, arr in weights.items():
            a = np.ascontiguousarray(arr, dtype=np.float32)
            dims = (ctypes.c_int64 * a.ndim)(*a.shape)
            self._check(self._lib.film_set_weight(self._h, name.encode(), a.ctypes.data, dims, a.ndim))
        self._check(self._lib.film_finalize(self._h))
        self._load_tune_cache()

    def load_bundle(self, path: str, verify: bool = True) -> Dict[str, Tuple[str, str]]:
        """film_load_bundle: reads the variables bundle of a Keras SavedModel directory (or a bundle prefix) natively - the
        replacement of tf.saved_model.load's variable restore, eval/interpolator.py:148 - places every tensor and finalizes.
        Returns {canonical name: (rule, checkpoint key)}, rule = 'path' | 'shape'; tensors placed by their (unique) shape are
        logged as a warning (a name match they are not)."""
        need = ctypes.c_int64()
        buf = ctypes.create_string_buffer(1 << 16)
        self._check(self._lib.film_load_bundle(self._h, os.fsencode(path), 1 if verify else 0, buf, len(buf), ctypes.byref(need)))
        if need.value > len(buf):    # the report did not fit (long checkpoint keys): read the bundle once more with a buffer that holds it
            buf = ctypes.create_string_buffer(int(need.value) + 1)
            self._check(self._lib.film_load_bundle(self._h, os.fsencode(path), 1 if verify else 0, buf, len(buf), ctypes.byref(need)))
        rep = {}
        # (checkpoint keys are bytes of the file: with verify=False a damaged index can hand back anything)
        for line in buf.value.decode('utf-8', 'replace').splitlines():
            parts = line.split('\t')
            if len(parts) == 3:
                rep[parts[0]] = (parts[1], parts[2])
        by_shape = sorted(n for n, (rule, _) in rep.items() if rule != 'path')
        if by_shape:
            import logging
            logging.getLogger('film_hip.tf_bundle').warning(
                '%s: %d of %d tensors were not found under a known object-graph path and were placed by their (unique) shape: %s',
                path, len(by_shape), len(rep), ', '.join(f'{n} <- {rep[n][1] if len(rep[n][1]) <= 160 else rep[n][1][:157] + "..."}' for n in by_shape))
        self._load_tune_cache()
        return rep

    # -- autotune choices across processes ($FILM_TUNE_CACHE = a file path) --------------------------------
    def export_tune(self) -> str:
        need = ctypes.c_int64()
        self._check(self._lib.film_export_tune(self._h, None, 0, ctypes.byref(need)))
        buf = ctypes.create_string_buffer(need.value)
        self._check(self._lib.film_export_tune(self._h, buf, need.value, ctypes.byref(need)))
        return buf.value.decode()

    def import_tune(self, text: str) -> None:
        self._check(self._lib.film_import_tune(self._h, text.encode()))

    def _load_tune_cache(self) -> None:
        path = os.environ.get('FILM_TUNE_CACHE')
        self._tune_saved = None
        if path and os.path.isfile(path):
            try:
                with open(path) as f:
                    self.import_tune(f.read())
                self._tune_saved = self.export_tune()
            except (OSError, FilmError):
                pass      # an unreadable / malformed cache only costs the measurements again

    def save_tune_cache(self) -> None:
        """Writes the autotune choices to $FILM_TUNE_CACHE if they changed (atomic rename; called after every
        host-buffer forward, call it yourself after warming up a device-resident pipeline)."""
        path = os.environ.get('FILM_TUNE_CACHE')
        if not path or self.device < 0:
            return
        text = self.export_tune()
        if text == getattr(self, '_tune_saved', None):
            return
        tmp = f'{path}.{os.getpid()}.tmp'
        try:
            with open(tmp, 'w') as f:
                f.write(text)
            os.replace(tmp, path)
            self._tune_saved = text
        except OSError:
            pass

    def packed_size(self) -> int:
        n = ctypes.c_int64()
        self._check(self._lib.film_packed_size(self._h, ctypes.byref(n)))
        return n.value

    def export_packed(self) -> np.ndarray:
        out = np.empty(self.packed_size(), dtype=np.float32)
        self._check(self._lib.film_export_packed(self._h, out.ctypes.data, out.size, FILM_MEM_HOST))
        return out

    def export_layouts(self) -> np.ndarray:
        """The kernel-layout blob packed so far (tests / debug; offsets as in plan())."""
        n = ctypes.c_int64()
        self._check(self._lib.film_export_layouts(self._h, None, 0, ctypes.byref(n)))
        out = np.empty(n.value, dtype=np.float32)
        self._check(self._lib.film_export_layouts(self._h, out.ctypes.data, out.size, ctypes.byref(n)))
        return out

    def import_packed(self, blob: np.ndarray) -> None:
        b = np.ascontiguousarray(blob, dtype=np.float32)
        self._check(self._lib.film_import_packed(self._h, b.ctypes.data, b.size, FILM_MEM_HOST))
        self._load_tune_cache()

    def import_packed_device(self, ptr: int, n_floats: int) -> None:
        self._check(self._lib.film_import_packed(self._h, ctypes.c_void_p(ptr), n_floats, FILM_MEM_DEVICE))
        self._load_tune_cache()

    def export_packed_device(self, ptr: int, n_floats: int) -> None:
        self._check(self._lib.film_export_packed(self._h, ctypes.c_void_p(ptr), n_floats, FILM_MEM_DEVICE))

    def bcast_weights(self, nccl_comm: int, root: int, rank: int, stream: int = 0) -> None:
        """film_bcast_weights: the RCCL broadcast of the parameter blob behind the C-ABI, over the CALLER's ncclComm_t (an integer
        handle here) - for hosts without torch.distributed; film_hip/sharding.py::broadcast_weights is the torch.distributed route."""
        self._check(self._lib.film_bcast_weights(self._h, ctypes.c_void_p(nccl_comm), root, rank, ctypes.c_void_p(stream)))
        if rank != root:
            self._load_tune_cache()

    # -- compute ----------------------------------------------------------------------------
    def forward(self, x0: np.ndarray, x1: np.ndarray) -> np.ndarray:
        """x0, x1: float32 [B,H,W,3] host arrays -> [B,H,W,3] (un-clipped), t = 0.5."""
        x0 = np.ascontiguousarray(x0, dtype=np.float32)
        x1 = np.ascontiguousarray(x1, dtype=np.float32)
        if x0.ndim != 4 or x0.shape[3] != 3 or x0.shape != x1.shape:
            raise ValueError(f'expected two [B,H,W,3] arrays of equal shape, got {x0.shape} and {x1.shape}')
        b, h, w, _ = x0.shape
        out = np.empty_like(x0)
        self._check(self._lib.film_forward(self._h, x0.ctypes.data, x1.ctypes.data, b, h, w,
                                           out.ctypes.data, FILM_MEM_HOST, None))
        self.save_tune_cache()
        return out

    def forward_device(self, x0_ptr: int, x1_ptr: int, b: int, h: int, w: int, out_ptr: int,
                       stream: Optional[int] = None) -> None:
        """Device-resident variant: raw device pointers (e.g. torch.Tensor.data_ptr()); asynchronous
        on `stream` (a hipStream_t as int, e.g. torch.cuda.current_stream().cuda_stream)."""
        self._check(self._lib.film_forward(self._h, ctypes.c_void_p(x0_ptr), ctypes.c_void_p(x1_ptr), b, h, w,
                                           ctypes.c_void_p(out_ptr), FILM_MEM_DEVICE,
                                           ctypes.c_void_p(stream) if stream else None))

    def interpolate_frames(self, x0: np.ndarray, x1: np.ndarray, align: Optional[int] = None,
                           block_shape=None, out: Optional[np.ndarray] = None) -> np.ndarray:
        """Interpolator.__call__ semantics in one C-ABI call (film_interpolate): pad to `align`, optional
        block_shape = (bh, bw) tiling with per-patch padding, crop, stitch - all on the device.
        `out`: an optional C-contiguous float32 array of x0's shape to receive the frame (a caller that reuses one - pinned, see
        torch_io.pinned_frame - saves the page faults of a fresh 25 MB array per call); default: a new array, like the reference."""
        x0 = np.ascontiguousarray(x0, dtype=np.float32)
        x1 = np.ascontiguousarray(x1, dtype=np.float32)
        if x0.ndim != 4 or x0.shape[3] != 3 or x0.shape != x1.shape:
            raise ValueError(f'expected two [B,H,W,3] arrays of equal shape, got {x0.shape} and {x1.shape}')
        b, h, w, _ = x0.shape
        bh, bw = (int(block_shape[0]), int(block_shape[1])) if block_shape else (1, 1)
        if out is None:
            out = np.empty_like(x0)
        elif out.dtype != np.float32 or out.shape != x0.shape or not out.flags['C_CONTIGUOUS'] or not out.flags['WRITEABLE']:
            raise ValueError(f'out must be a writable C-contiguous float32 array of shape {x0.shape}')
        self._check(self._lib.film_interpolate(self._h, x0.ctypes.data, x1.ctypes.data, b, h, w, int(align or 0),
                                               bh, bw, out.ctypes.data, FILM_MEM_HOST, None))
        self.save_tune_cache()
        return out

    def interpolate_frames_device(self, x0_ptr: int, x1_ptr: int, b: int, h: int, w: int, out_ptr: int,
                                  align: Optional[int] = None, block_shape=None, stream: Optional[int] = None) -> None:
        """Device-resident film_interpolate: raw device pointers, asynchronous on `stream`."""
        bh, bw = (int(block_shape[0]), int(block_shape[1])) if block_shape else (1, 1)
        self._check(self._lib.film_interpolate(self._h, ctypes.c_void_p(x0_ptr), ctypes.c_void_p(x1_ptr), b, h, w,
                                               int(align or 0), bh, bw, ctypes.c_void_p(out_ptr), FILM_MEM_DEVICE,
                                               ctypes.c_void_p(stream) if stream else None))

    def interpolate_sequence(self, frames: np.ndarray, align: Optional[int] = None, block_shape=None,
                             out: Optional[np.ndarray] = None) -> np.ndarray:
        """Mid-frames of every consecutive pair of a frame sequence (film_interpolate_sequence): frames float32 [F,H,W,3], F >= 2
        -> [F-1,H,W,3], out[j] bit-identical to interpolate_frames(frames[:-1], frames[1:], align, block_shape)[j], with one feature
        extraction per frame instead of two per pair.  `out` as for interpolate_frames (shape [F-1,H,W,3])."""
        frames = np.ascontiguousarray(frames, dtype=np.float32)
        if frames.ndim != 4 or frames.shape[3] != 3:
            raise ValueError(f'expected a [F,H,W,3] array, got {frames.shape}')
        f, h, w, _ = frames.shape
        bh, bw = (int(block_shape[0]), int(block_shape[1])) if block_shape else (1, 1)
        shape = (max(f - 1, 0), h, w, 3)
        if out is None:
            out = np.empty(shape, np.float32)
        elif out.dtype != np.float32 or out.shape != shape or not out.flags['C_CONTIGUOUS'] or not out.flags['WRITEABLE']:
            raise ValueError(f'out must be a writable C-contiguous float32 array of shape {shape}')
        self._check(self._lib.film_interpolate_sequence(self._h, frames.ctypes.data, f, h, w, int(align or 0), bh, bw,
                                                        out.ctypes.data, FILM_MEM_HOST, None))
        self.save_tune_cache()
        return out

    def interpolate_sequence_device(self, frames_ptr: int, f: int, h: int, w: int, out_ptr: int, align: Optional[int] = None,
                                    block_shape=None, stream: Optional[int] = None) -> None:
        """Device-resident film_interpolate_sequence: frames [f,h,w,3] -> out [f-1,h,w,3] (raw device pointers), asynchronous on `stream`."""
        bh, bw = (int(block_shape[0]), int(block_shape[1])) if block_shape else (1, 1)
        self._check(self._lib.film_interpolate_sequence(self._h, ctypes.c_void_p(frames_ptr), f, h, w, int(align or 0), bh, bw,
                                                        ctypes.c_void_p(out_ptr), FILM_MEM_DEVICE,
                                                        ctypes.c_void_p(stream) if stream else None))

    def open_stream(self, h: int, w: int, align: Optional[int] = None, block_shape=None, pix: str = 'f32', matrix: str = 'bt709',
                    full_range: bool = False, scene_cut: int = 0, times: int = 1, dedup=None) -> FilmStream:
        """film_stream_open: a frame stream of h x w frames, padded / tiled like interpolate_frames(align, block_shape); pix is a name of
        film_hip/pixfmt.py's table (FilmStream describes the frames; 4:2:0 needs h and w even, 4:2:2 w even), the Y'CbCr ones with the colour
        `matrix` 'bt709' | 'bt601' | 'bt2020nc' and limited or full range.
        scene_cut: 0 .. 1000 permille; non-zero sets the engine option "scene_cut" (include/film_hip.h) before the stream opens - a handle
        option like block_overlap, so it STAYS set for later streams of this engine until set_option('scene_cut', 0); 0 (default) leaves
        the engine as it is.
        times: 1 .. 6 = the engine option "stream_times" for THIS stream (set, the stream opened, the option set back to what it was): a
        primed push returns the 2^times - 1 frames of the times_to_interpolate recursion (FilmStream).
        dedup: None (default) leaves the engine as it is; hi, or (hi, lo, frac), sets the engine options "dup_hi", "dup_lo" and "dup_frac"
        (include/film_hip.h, "Duplicate frames"; hi alone: lo = 0, frac = 1000) before the stream opens - handle options like scene_cut, so
        they STAY set for later streams of this engine until set_option('dup_hi', -1).  A push judged a duplicate of the carried frame then
        returns None / False and changes nothing; FilmStream.dup_info() tells it from a first push or a cut."""
        if scene_cut:
            self.set_option('scene_cut', int(scene_cut))
        if dedup is not None:
            for key, v in zip(('dup_hi', 'dup_lo', 'dup_frac'), dedup_options(dedup)):
                self.set_option(key, v)
        times = int(times)
        before = getattr(self, '_stream_times', 1)   # (option "stream_times" as last set through set_option)
        if times == before:
            return FilmStream(self, h, w, align, block_shape, pix, matrix, full_range, times)
        self.set_option('stream_times', times)
        try:
            return FilmStream(self, h, w, align, block_shape, pix, matrix, full_range, times)
        finally:
            self.set_option('stream_times', before)

    def frame_histogram_device(self, ptr: int, h: int, w: int, hist_ptr: int, pix: str = 'u8', matrix: str = 'bt709', full_range: bool = False,
                               stream: Optional[int] = None) -> None:
        """film_frame_histogram on raw device pointers (the module function frame_histogram_device: the call needs no handle)."""
        frame_histogram_device(ptr, h, w, hist_ptr, pix, matrix, full_range, stream)

    @staticmethod
    def _metric_flags(names, clip: bool) -> int:
        unknown = [n for n in names if n not in METRIC_FLAGS]
        if unknown:
            raise ValueError(f'film_image_metrics computes {sorted(METRIC_FLAGS)}, not {unknown}')
        flags = FILM_METRIC_CLIP if clip else 0
        for n in names:
            flags |= METRIC_FLAGS[n]
        return flags

    def image_metrics(self, pred: np.ndarray, ref: np.ndarray, names=('l1', 'l2', 'ssim', 'psnr'), clip: bool = False,
                      max_val: float = 1.0) -> np.ndarray:
        """film_image_metrics on host arrays: pred, ref float32 [B,H,W,C] (or [H,W,C]), C = 1 or 3 -> float64 [B,4] per image:
        sum |d| and sum d*d of the float32 difference d, psnr in dB, ssim; NaN where the metric is not in `names`.  clip: pred is
        clipped to [0,1] first.  eval.device_metrics.compose turns these into the values of eval/metrics.py."""
        pred = np.ascontiguousarray(pred, dtype=np.float32)
        ref = np.ascontiguousarray(ref, dtype=np.float32)
        if pred.ndim == 3:
            pred, ref = pred[None], ref[None]
        if pred.ndim != 4 or pred.shape != ref.shape:
            raise ValueError(f'expected two [B,H,W,C] arrays of equal shape, got {pred.shape} and {ref.shape}')
        b, h, w, c = pred.shape
        out = np.empty((b, 4), np.float64)
        self._check(self._lib.film_image_metrics(self._h, pred.ctypes.data, ref.ctypes.data, b, h, w, c,
                                                 self._metric_flags(names, clip), float(max_val), out.ctypes.data,
                                                 FILM_MEM_HOST, None))
        return out

    def image_metrics_device(self, pred_ptr: int, ref_ptr: int, b: int, h: int, w: int, c: int,
                             names=('l1', 'l2', 'ssim', 'psnr'), clip: bool = False, max_val: float = 1.0,
                             stream: Optional[int] = None) -> np.ndarray:
        """image_metrics on device pointers ([b,h,w,c] float32 each) on `stream` (ordered after the work queued there before);
        returns the same float64 [b,4] host array once the stream has reached the end of the call."""
        out = np.empty((int(b), 4), np.float64)
        self._check(self._lib.film_image_metrics(self._h, ctypes.c_void_p(pred_ptr), ctypes.c_void_p(ref_ptr), int(b), int(h),
                                                 int(w), int(c), self._metric_flags(names, clip), float(max_val),
                                                 out.ctypes.data, FILM_MEM_DEVICE, ctypes.c_void_p(stream) if stream else None))
        return out

    def to_uint8_device(self, src_ptr: int, dst_ptr: int, n: int, stream: Optional[int] = None) -> None:
        """film_to_uint8: write_image's quantisation (eval/util.py:51-52) of n device floats into n device bytes, asynchronous."""
        rc = self._lib.film_to_uint8(ctypes.c_void_p(src_ptr), ctypes.c_void_p(dst_ptr), int(n), ctypes.c_void_p(stream) if stream else None)
        if rc != 0:
            raise FilmError(rc, 'film_to_uint8 failed')

    def _to_yuv(self, symbol: str, src_ptr, dst_ptr, h, w, pix, matrix, full_range, stream) -> None:
        rc = getattr(self._lib, symbol)(ctypes.c_void_p(src_ptr), ctypes.c_void_p(dst_ptr), int(h), int(w), pix_code(pix, matrix, full_range),
                                        ctypes.c_void_p(stream) if stream else None)
        if rc != 0:
            raise FilmError(rc, f'{symbol} failed')

    def to_yuv420_device(self, src_ptr: int, dst_ptr: int, h: int, w: int, pix: str = 'i420', matrix: str = 'bt709',
                         full_range: bool = False, stream: Optional[int] = None) -> None:
        """film_to_yuv420: h x w x 3 device floats -> one 4:2:0 frame of h * w * 3 // 2 device bytes, or 16-bit words for the 10-bit layouts
        (dst_ptr 2-byte aligned), asynchronous."""
        self._to_yuv('film_to_yuv420', src_ptr, dst_ptr, h, w, pix, matrix, full_range, stream)

    def to_yuv_device(self, src_ptr: int, dst_ptr: int, h: int, w: int, pix: str = 'i444', matrix: str = 'bt709',
                      full_range: bool = False, stream: Optional[int] = None) -> None:
        """film_to_yuv: h x w x 3 device floats -> one frame of ANY Y'CbCr layout (4:2:0, 4:2:2, 4:4:4; device bytes, or 16-bit words for the
        10-bit layouts: dst_ptr 2-byte aligned), asynchronous."""
        self._to_yuv('film_to_yuv', src_ptr, dst_ptr, h, w, pix, matrix, full_range, stream)

    def set_option(self, key: str, value: int) -> None:
        self._check(self._lib.film_set_option(self._h, key.encode(), int(value)))
        if key == 'stream_times':
            self._stream_times = int(value)
        if key in ('block_overlap_h', 'block_overlap_w'):
            self._block_overlap = tuple(int(value) if key == k else o
                                        for k, o in zip(('block_overlap_h', 'block_overlap_w'), self.block_overlap))

    @property
    def block_overlap(self) -> Tuple[int, int]:
        """The (height, width) values of options "block_overlap_h" / "block_overlap_w" as last set (0: disjoint patches; -1: what the
        align padding holds); what they resolve to for a frame size: tiling()."""
        return getattr(self, '_block_overlap', (0, 0))

    def set_block_overlap(self, block_overlap) -> None:
        """block_overlap: an int for both axes or (height, width) - sets the two options."""
        oh, ow = (block_overlap, block_overlap) if np.isscalar(block_overlap) else block_overlap
        self.set_option('block_overlap_h', int(oh))
        self.set_option('block_overlap_w', int(ow))

    # -- introspection ------------------------------------------------------------------------
    def _json_call(self, fn, *args) -> dict:
        need = ctypes.c_int64()
        self._check(fn(self._h, *args, None, 0, ctypes.byref(need)))
        buf = ctypes.create_string_buffer(need.value)
        self._check(fn(self._h, *args, buf, need.value, ctypes.byref(need)))
        return json.loads(buf.value.decode())

    def plan(self, b: int, h: int, w: int) -> dict:
        return self._json_call(self._lib.film_plan_json, b, h, w)

    def sequence_plan(self, n_pairs: int, tiles: int, h: int, w: int) -> dict:
        """film_sequence_plan_json: the plan film_interpolate_sequence runs for n_pairs consecutive pairs of `tiles` h x w tiles."""
        return self._json_call(self._lib.film_sequence_plan_json, n_pairs, tiles, h, w)

    def stream_plan(self, tiles: int, h: int, w: int, slot: int) -> dict:
        """film_stream_plan_json: the plan a stream of `tiles` h x w tiles runs when the pushed frame fills half `slot` (0 / 1)."""
        return self._json_call(self._lib.film_stream_plan_json, int(tiles), int(h), int(w), int(slot))

    def stream_pair_plan(self, tiles: int, h: int, w: int, times: int, left: int, right: int, extract: bool = True) -> dict:
        """film_stream_pair_plan_json: the plan of one pair run (frame in slot `left`, frame in slot `right`, with or without the right
        frame's extraction) of a stream of `tiles` h x w tiles opened with times (times + 1 frame slots)."""
        return self._json_call(self._lib.film_stream_pair_plan_json, int(tiles), int(h), int(w), int(times), int(left), int(right), int(bool(extract)))

    def stream_group_schedule(self, tiles: int, h: int, w: int, times: int, slot: int, group_tiles: int, select=None) -> dict:
        """film_stream_group_schedule_json: the runs of one primed push (select as for stream_schedule; an empty selection: a first push) of
        a stream whose frame of `tiles` h x w tiles runs in groups of group_tiles - per step and group the restores from the carry, where the
        extracted frame comes from, the run, the save and the joined tile range (include/film_hip.h, "Tile groups")."""
        return self._json_call(self._lib.film_stream_group_schedule_json, int(tiles), int(h), int(w), int(times), int(slot),
                               selection_mask(times, select), int(group_tiles))

    def stream_schedule(self, times: int, slot: int, select=None) -> dict:
        """film_stream_schedule_json: the pair runs of one primed push whose input lands in slot 0 / 1, in execution order.  select (an
        iterable of 1-based positions, FilmStream.select): film_stream_select_schedule_json - the steps of the push with that selection,
        each with "deliver" and "run" ('pair' | 'extract')."""
        if select is None:
            return self._json_call(self._lib.film_stream_schedule_json, int(times), int(slot))
        if not 1 <= int(times) <= 6:
            raise ValueError(f'times must be 1 .. 6, got {times}')
        return self._json_call(self._lib.film_stream_select_schedule_json, int(times), int(slot), selection_mask(times, select))

    def tiling(self, h: int, w: int, align: Optional[int] = None, block_shape=None) -> dict:
        """film_tiling_json: the tile geometry of an h x w frame with the engine's current block_overlap options (resolved overlap,
        tile content and padded size, pad offsets, tile origins per axis); refuses what the compute calls refuse.  Needs no GPU."""
        bh, bw = (int(block_shape[0]), int(block_shape[1])) if block_shape else (1, 1)
        return self._json_call(self._lib.film_tiling_json, int(h), int(w), int(align or 0), bh, bw)

    def profile(self) -> dict:
        return self._json_call(self._lib.film_profile_json)

    def tap(self, name: str) -> np.ndarray:
        dims = (ctypes.c_int64 * 4)()
        self._check(self._lib.film_get_tap(self._h, name.encode(), None, 0, dims))
        shape = tuple(int(d) for d in dims)
        out = np.empty(shape, dtype=np.float32)
        self._check(self._lib.film_get_tap(self._h, name.encode(), out.ctypes.data, out.size, dims))
        return out

    # -- debug / tests: one planned launch on a workspace the caller controls ---------------------------------
    def debug_arena_write(self, key, offset: int, data: np.ndarray) -> None:
        """film_debug_arena, host -> workspace: key = (B, H, W) or (B, H, W, tiles) of the device plan, data float32."""
        b, h, w, tiles = (tuple(key) + (0,))[:4]
        a = np.ascontiguousarray(data, dtype=np.float32)
        self._check(self._lib.film_debug_arena(self._h, b, h, w, tiles, int(offset), a.size, a.ctypes.data, 1))

    def debug_arena_read(self, key, offset: int, count: int) -> np.ndarray:
        """film_debug_arena, workspace -> host: `count` floats from float offset `offset`."""
        b, h, w, tiles = (tuple(key) + (0,))[:4]
        out = np.empty(int(count), np.float32)
        self._check(self._lib.film_debug_arena(self._h, b, h, w, tiles, int(offset), out.size, out.ctypes.data, 0))
        return out

    def debug_run_op(self, key, index: int, candidate: int = -1) -> int:
        """film_debug_run_op: launches op `index` of the plan once (candidate -1: the plan's tile, k >= 0: entry k of the op's
        autotune candidate list) and returns the length of that list (0 for ops that are no convolutions)."""
        b, h, w, tiles = (tuple(key) + (0,))[:4]
        n = ctypes.c_int(0)
        self._check(self._lib.film_debug_run_op(self._h, b, h, w, tiles, int(index), int(candidate), ctypes.byref(n)))
        return n.value

    def debug_tile_map(self, mode: str, frames_ptr: int, tiles_ptr: int, b: int, h: int, w: int, align: Optional[int], block_shape,
                       tile0: int, ntiles: int, u8: bool = False, stream: Optional[int] = None) -> None:
        """film_debug_tile_map: ONE cut (mode 'cut': frames -> tiles) or join ('join': tiles -> frames) of tiles [tile0, tile0 + ntiles)
        of b frames [b,h,w,3] on device pointers the caller owns, with the geometry of tiling(h, w, align, block_shape); tile n sits at
        index n - tile0 of the tile buffer.  u8 (cut only): the frames are bytes in a 4-byte aligned allocation of whole 32-bit words.
        Asynchronous on `stream` (default stream when None)."""
        bh, bw = (int(block_shape[0]), int(block_shape[1])) if block_shape else (1, 1)
        self._check(self._lib.film_debug_tile_map(self._h, {'cut': 0, 'join': 1}[mode], pix_code('u8' if u8 else 'f32'),
                                                  ctypes.c_void_p(frames_ptr), ctypes.c_void_p(tiles_ptr), int(b), int(h), int(w),
                                                  int(align or 0), bh, bw, int(tile0), int(ntiles),
                                                  ctypes.c_void_p(stream) if stream else None))

    def debug_yuv_cut(self, frames_ptr: int, tiles_ptr: int, b: int, h: int, w: int, align: Optional[int], block_shape, tile0: int,
                      ntiles: int, pix: str = 'i420', matrix: str = 'bt709', full_range: bool = False, stream: Optional[int] = None) -> None:
        """film_debug_yuv_cut: ONE cut of tiles [tile0, tile0 + ntiles) of b 4:2:0 frames (h * w * 3 // 2 samples each, in a 4-byte aligned
        allocation of whole 32-bit words) into float32 RGB tiles, with the geometry of tiling(h, w, align, block_shape)."""
        bh, bw = (int(block_shape[0]), int(block_shape[1])) if block_shape else (1, 1)
        self._check(self._lib.film_debug_yuv_cut(self._h, pix_code(pix, matrix, full_range), ctypes.c_void_p(frames_ptr),
                                                 ctypes.c_void_p(tiles_ptr), int(b), int(h), int(w), int(align or 0), bh, bw, int(tile0),
                                                 int(ntiles), ctypes.c_void_p(stream) if stream else None))

    def forward_with_aux(self, x0: np.ndarray, x1: np.ndarray) -> Dict[str, object]:
        """The reference model's output dictionary with `use_aux_outputs` on (models/film_net/interpolator.py:
        188-199): 'image', 'x0_warped', 'x1_warped' and the four flow pyramids (lists, finest level first), read
        back from the workspace of this forward.  H, W must already be divisible by 2^(pyramid_levels-1)."""
        from . import weights as W
        image = self.forward(x0, x1)
        b = image.shape[0]
        opt = self.options
        c0 = W.feature_channels(opt)[0]
        aligned0 = self.tap('aligned0')
        res = [self.tap(f'res{l}') for l in range(opt.pyramid_levels)]
        flow = [self.tap(f'v{l}') if l < opt.pyramid_levels - 1 else res[l] for l in range(opt.fusion_pyramid_levels)]
        return {
            'image': image,
            'x0_warped': np.ascontiguousarray(aligned0[..., 2 * c0:2 * c0 + 3]),
            'x1_warped': np.ascontiguousarray(aligned0[..., 2 * c0 + 3:2 * c0 + 6]),
            'forward_residual_flow_pyramid': [r[:b] for r in res],
            'backward_residual_flow_pyramid': [r[b:] for r in res],
            'forward_flow_pyramid': [f[:b] for f in flow],
            'backward_flow_pyramid': [f[b:] for f in flow],
        }

    @staticmethod
    def version() -> str:
        return load_library().film_version().decode()

    @staticmethod
    def has_extra_families() -> bool:
        """True for a FILM_EXTRA_FAMILIES=1 build: the precision modes and the winograd = 2 / halo_all options exist."""
        return '+extra' in FilmEngine.version()
