/*
 * film_hip.h  --  C-ABI of libfilm_hip.so, the MI355X (gfx950) FILM inference engine.
 *
 * This is the drop-in boundary for the reference's one operator call on the hot path:
 *
 *     self._model = tf.compat.v2.saved_model.load(model_path)        eval/interpolator.py:148
 *     result = self._model({'x0','x1','time'}, training=False)       eval/interpolator.py:170-171
 *     image  = result['image']                                       eval/interpolator.py:172
 *
 * i.e. "load the film_net weights" and "run models/film_net (interpolator.py:89-207) on a
 * batch of frame pairs and return the t=0.5 frame".  Everything here is plain C: pointers
 * and sizes, no torch / numpy types.  The Python host
 * (frame-interpolation_amd/eval/interpolator.py) binds it with ctypes; INTEGRATION.md shows
 * the stub a maintainer of the reference would add.
 *
 * Tensors are NHWC float32, weights are TF HWIO [kh,kw,cin,cout] float32 (the layout a
 * Keras SavedModel stores, training/train_lib.py:280).
 *
 * Every function returns 0 on success or a negative FILM_ERR_* code; the message is
 * available from film_last_error().  A handle owns one device, one stream, the packed
 * weights and a per-(B,H,W) cached execution plan + workspace.  Handles are not
 * thread-safe - ONE in-flight issuer per handle: a forward launches on the caller's stream and on
 * the handle's side stream with one set of events per plan, so two threads (or two streams) must
 * not issue forwards of the same handle concurrently.  Several handles may coexist, also on
 * several host threads (tests/test_host_threads_cpu.py runs that under ThreadSanitizer).
 */
#ifndef FILM_HIP_H_
#define FILM_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FILM_OK 0
#define FILM_ERR_INVALID (-1)    /* bad argument / shape (reference: assert / ValueError)      */
#define FILM_ERR_STATE (-2)      /* call order (e.g. forward before finalize)                   */
#define FILM_ERR_NO_DEVICE (-3)  /* no HIP device: the engine has NO CPU fallback               */
#define FILM_ERR_HIP (-4)        /* a HIP runtime call failed                                   */
#define FILM_ERR_NOMEM (-5)
#define FILM_ERR_NOTFOUND (-6)   /* unknown weight / tap name                                   */

#define FILM_MEM_HOST 0   /* x0/x1/out are host pointers: H2D + D2H done by the call          */
#define FILM_MEM_DEVICE 1 /* x0/x1/out are device pointers on the handle's device              */

#define FILM_MAX_SPECIALIZED 7

typedef struct film_handle film_t;

/* models/film_net/options.py:20-80 ; defaults = training/config/film_net-L1.gin:17-23 */
typedef struct film_config {
  int32_t pyramid_levels;
  int32_t fusion_pyramid_levels;
  int32_t specialized_levels;
  int32_t sub_levels;
  int32_t filters;
  int32_t flow_convs[FILM_MAX_SPECIALIZED + 1];   /* specialized_levels+1 entries used */
  int32_t flow_filters[FILM_MAX_SPECIALIZED + 1]; /* specialized_levels+1 entries used */
} film_config;

/* Fills *cfg with the published architecture (film_net-L1.gin:17-23). */
int film_default_config(film_config* cfg);

/* Creates an engine on HIP device `device` (>= 0).
 * device == -1 creates a PLAN-ONLY handle: it can take weights, pack them and describe
 * plans (film_plan_json / film_export_packed) without a GPU, and every compute entry point
 * returns FILM_ERR_NO_DEVICE.  There is no CPU execution path in this library.
 * Replaces: tf.compat.v2.saved_model.load (eval/interpolator.py:148), object creation half. */
int film_create(film_t** out, int device, const film_config* cfg);
void film_destroy(film_t* h);

/* Message of the last failing call on this handle (or of film_create when h == NULL). */
const char* film_last_error(const film_t* h);

/* Supplies one tensor by canonical name, e.g.
 *   "feat_net/sub_extractor/cfeat_conv_0/kernel"  dims = {3,3,3,64}
 *   "predict_flow/flow_predictor_shared/conv_4/bias"  dims = {2}
 * (names: frame-interpolation_amd/film_hip/weights.py).  Data is copied.
 * Replaces: the variable restore inside saved_model.load (eval/interpolator.py:148). */
int film_set_weight(film_t* h, const char* name, const float* data, const int64_t* dims, int ndim);

/* Checks that every tensor of the architecture is present with the right shape, repacks
 * HWIO into the engine's K-major layout (zero-padding / permuting concat segments) and
 * uploads the blob to the device. */
int film_finalize(film_t* h);

/* The parameter set as ONE flat blob of floats - per layer, in layer order, the HWIO kernel then the bias (137.7 MB for the
 * published net): size, export to / import from a caller buffer.  This is what ranks exchange: rank 0 reads the model,
 * the others receive the blob by RCCL broadcast and film_import_packed() it (= film_set_weight of every tensor +
 * film_finalize).  Kernel layouts are built per handle, on demand: film_finalize packs what the default fp32 plan reads
 * (K-major + F(4,3) + phase-summed 2x2 copies, 3.0x the parameters, multi-threaded, well under a second); the F(2,3), halo
 * and bf16-split copies are packed when an option or a plan first needs them. */
int film_packed_size(film_t* h, int64_t* n_floats);
int film_export_packed(film_t* h, float* dst, int64_t capacity_floats, int mem_kind);
int film_import_packed(film_t* h, const float* src, int64_t n_floats, int mem_kind);

/* The weight broadcast itself, for hosts without torch.distributed (north_star: "RCCL broadcast of weights over xGMI"; the
 * reference has nothing to replace here - every beam worker calls tf.saved_model.load on its own, eval/interpolator_cli.py:127-150).
 * Collective over `nccl_comm` (an ncclComm_t of the CALLER - the library creates no communicator and links no RCCL: ncclBroadcast is
 * resolved at run time from the RCCL already in the process, else from librccl.so): rank `root` must hold a finalized weight set and sends
 * the flat parameter blob (film_packed_size floats, staged in a device buffer of handle `h`'s GPU), every other rank receives it and
 * film_import_packed()s it (= film_finalize with the received set).  `rank` = the caller's rank in the communicator; `stream` = the HIP
 * stream the broadcast is enqueued on (NULL: the handle's own), synchronised before the function returns.  Every rank must call it. */
int film_bcast_weights(film_t* h, void* nccl_comm, int root, int rank, void* stream);

/* Debug / tests: the kernel-layout blob packed so far (offsets as in film_plan_json; "pack_groups" option packs more).
 * dst == NULL: size query. */
int film_export_layouts(film_t* h, float* dst, int64_t capacity_floats, int64_t* n_floats);

/* Runs film_net on B frame pairs: x0, x1 [B,H,W,3] -> out [B,H,W,3] (un-clipped), t = 0.5.
 * H and W must be divisible by 2^(pyramid_levels-1) (options.py:36-37) - pad first, as
 * Interpolator.interpolate does (eval/interpolator.py:166-168).
 * `stream`: a hipStream_t to run on.  NULL means: with FILM_MEM_HOST the handle's own stream (the call
 * synchronises before returning); with FILM_MEM_DEVICE the NULL (legacy default) stream, so the work
 * is ordered with the caller's default-stream work (PyTorch's default stream is the NULL stream) and
 * the call is asynchronous.
 * Replaces: self._model(inputs, training=False)['image'] (eval/interpolator.py:170-172). */
int film_forward(film_t* h, const float* x0, const float* x1, int B, int H, int W, float* out,
                 int mem_kind, void* stream);

/* Interpolator.__call__ on the device (eval/interpolator.py:178-209), frames x0, x1 [B,H,W,3] -> out [B,H,W,3]:
 *   block_h * block_w <= 1 : zero-pad H, W up to multiples of `align` (offset pad//2, _pad_to_align :30-63), run the
 *                            model, crop (Interpolator.interpolate :152-176);
 *   block_h * block_w  > 1 : split every frame into block_h x block_w row-major patches (image_to_patches
 *                            :66-99, same divisibility asserts), pad EACH patch to `align`, run all patches as one
 *                            batch (the reference loops over them with B = 1, :199-206), crop each, stitch
 *                            (patches_to_image :102-126).  The reference's tiled path takes one frame pair; B > 1
 *                            here tiles every pair of the batch the same way (used by the breadth-first
 *                            recursion driver, film_hip/recursive.py).
 * align <= 0 means no padding (the reference's align=None); H, W (or the patch) must then be divisible by
 * 2^(pyramid_levels-1).  Pad / patch / crop / stitch are two HIP kernels that read the caller's frames and write
 * the plan's input buffer directly (and back), so with FILM_MEM_DEVICE nothing but the frames themselves is copied.
 * Batches are processed in chunks of tiles that keep one invocation's workspace below 64 GiB (and below 60 % of the HBM the
 * handle can get at that moment) and every buffer read through a 32-bit whole-buffer offset below 4 GiB; the chunk is the
 * largest divisor of the tile count inside that bound where one exists, so every invocation replays one cached plan
 * (16 * 2^k tiles of a 4K recursion -> chunks of 8), and it is halved when a workspace allocation fails (results unchanged).
 * `stream` and mem_kind as for film_forward. */
int film_interpolate(film_t* h, const float* x0, const float* x1, int B, int H, int W, int align, int block_h,
                     int block_w, float* out, int mem_kind, void* stream);

/* film_interpolate over a frame SEQUENCE: frames [F,H,W,3] -> out [F-1,H,W,3], out[j] = the mid-frame of frames[j] and frames[j+1],
 * bit-identical to film_interpolate(frames[:-1], frames[1:], F - 1, ...).  The image pyramid and the feature extractor run once per
 * frame (F extractions instead of 2 (F - 1)): a sequence plan holds k consecutive pairs x nt tiles per invocation ((k + 1) * nt
 * image-tiles; the boundary frame is extracted again by the next chunk), pairs of different input pairs batch together.  Chunks are
 * bounded by the limits of film_interpolate and "max_batch" (counted in pair-tiles), prefer the most pairs per extracted image, then
 * whole frames, and are halved when a workspace allocation fails (results unchanged).  F < 2: FILM_ERR_INVALID.  align / block_h /
 * block_w / mem_kind / stream as for film_interpolate (same padding, tiling, asserts); FILM_MEM_HOST is upload, work, download
 * ("host_overlap" does not apply). */
int film_interpolate_sequence(film_t* h, const float* frames, int F, int H, int W, int align, int block_h, int block_w,
                              float* out, int mem_kind, void* stream);

/* Frame STREAMS: film_interpolate for a caller that receives its frames one at a time (a player, a transcoder, a capture card).  The
 * caller pushes one frame and gets the mid-frame between it and the frame pushed before; the earlier frame's image pyramid and feature
 * pyramid are read where that push left them, so every frame is extracted once (film_interpolate extracts every inner frame twice)
 * and nothing is copied between pushes: a stream plan holds the two frames of a pair in two slots that take turns.
 *   film_stream_open   H x W frames, align / block_h / block_w as for film_interpolate (same padding, tiling, "block_overlap_*",
 *                      refusals).  pix: a pixel type below (a layout, for the 4:2:0 layouts plus colour flags).  ONE open stream per handle (a second open: FILM_ERR_STATE);
 *                      several streams = several handles, as for threads.  Builds (and autotunes) the plan, so the pushes are steady.
 *                      A frame whose tiles fit ONE model invocation under the limits of film_interpolate runs in one ("one group": nothing
 *                      below applies, and a push makes the device calls it always made).  A frame of more tiles than an invocation takes
 *                      ("max_batch", the 4 GiB-per-buffer rule) or one whose workspace of "stream_times" + 1 slots does not fit - a 4K frame
 *                      cut 4 x 4 with "stream_times" >= 2 on a 288 GB device - runs in TILE GROUPS ("Tile groups"
 *                      below): n = the chunk film_interpolate would choose, halved while the workspace of n tiles does not fit; n and the
 *                      number of groups are fixed for the stream's life (a later "max_batch" does not touch an open stream).  FILM_ERR_NOMEM:
 *                      a single tile's workspace does not fit, or the groups' carry buffer cannot be allocated (the message names the
 *                      workspace bytes, the carry bytes, n and the groups); FILM_ERR_INVALID: a single tile too large for a 32-bit
 *                      addressed buffer.  Plan-only handle: FILM_ERR_NO_DEVICE; before film_finalize: FILM_ERR_STATE.
 *   film_stream_push   frame [H,W,3] in, mid [H,W,3] out, both of the stream's pixel type (a 4:2:0 stream: H * W * 3 / 2 samples each - bytes, or 16-bit words for the 10-bit layouts).  The first push after open / reset sets
 *                      *produced = 0 and only cuts the frame into its tiles and runs the image pyramid and the feature extractor
 *                      (`mid` is not touched and may be NULL); every later push sets *produced = 1 and writes `mid`, bit-identical
 *                      to film_interpolate(previous frame, frame, 1, H, W, align, block_h, block_w) under the handle's current
 *                      options - with FILM_PIX_U8 to film_to_uint8 of that call on the frames u8 / 255.0f, byte for byte; with a 4:2:0
 *                      pixel type to film_to_yuv420 of that call on the frames converted by "In" below, byte for byte.
 *                      mem_kind / stream as for film_interpolate; FILM_MEM_HOST is upload, work, download ("host_overlap" does not
 *                      apply) and moves one byte per value each way with FILM_PIX_U8.  Results never depend on what else the handle
 *                      did between two pushes: the stream keeps its own device copy of the previous frame and extracts it again,
 *                      silently and with the same bits, when its plan was evicted or dropped meanwhile.  After a push that fails
 *                      the stream is as after film_stream_reset, and both of the handle's streams are drained before the error returns.
 *   film_stream_reset  forgets the carried frame (scene cut, seek): the next push produces nothing.
 *   film_stream_cut_info  what the last push found with option "scene_cut" (below, "Scene cuts"): *distance = D between the pushed frame and
 *                      the one before, or -1 when no comparison was made (the option is 0, the first frame, the push after a reset or after a
 *                      failed push, the first push after the option was turned on); *samples = S of one frame; *cut = 1 when the push
 *                      was treated as a scene cut, else 0.  NULL outputs are skipped.
 *   film_stream_dup_info  what the last push found with option "dup_hi" (below, "Duplicate frames"): the block statistics of the pushed frame
 *                      against the carried one, and whether the push was dropped as a duplicate (it then set *produced = 0 and changed nothing).
 *   film_stream_close  frees the stream's buffers (film_destroy closes an open stream too).
 * push / reset / close without an open stream: FILM_ERR_STATE.
 *   film_stream_plan_json  the stream plan of `tiles` (padded) H x W tiles in orientation `slot` (0 / 1: the half of the frame buffers
 *                      the pushed frame fills; pushes alternate) as film_plan_json text with "kind":"stream", "tiles", "slot",
 *                      "n_extract": B = tiles, img0 / the feature buffers hold 2 * tiles images, ops [0, n_extract) are the pushed
 *                      frame's image pyramid and extractor (all a first push runs), the rest is the sequence plan of one pair with the
 *                      earlier frame at image (1 - slot) * tiles.  Both orientations list the same buffers.  Works on plan-only handles.
 *                      Always the two-slot plan of "stream_times" = 1, whatever the option says.
 * Recursive mid-frames (option "stream_times" = T, 1 .. 6, default 1; read by film_stream_open and fixed for that stream's life).  With T > 1
 * a primed film_stream_push writes the 2^T - 1 frames of the reference's times_to_interpolate = T recursion (eval/util.py,
 * _recursive_generator) between the previous frame and the pushed one to `mid`: contiguous frames of the stream's pixel type in temporal
 * order, `mid` holding (2^T - 1) frames, *produced = 2^T - 1.  A first push, a push after film_stream_reset and a scene-cut push write
 * nothing and set *produced = 0, as with T = 1; a NULL `mid` on a primed push is FILM_ERR_INVALID and unprimes the stream.
 *   Definition.  With the previous frame at position 0 and the pushed one at 2^T, the frame at position (2 j + 1) 2^(T - d), d = 1 .. T, is
 *     film_interpolate of the frames at positions (2 j) 2^(T - d) and (2 j + 2) 2^(T - d) - its two depth-(d - 1) neighbours - as FLOAT32
 *     frames: a mid-frame that is fed back is never quantised on the way.  A FILM_PIX_F32 stream returns these floats, a FILM_PIX_U8 stream
 *     film_to_uint8 of them, a 4:2:0 stream film_to_yuv420 of them; the inputs are dequantised once, by the cut.  Every output is therefore
 *     bit-identical to pairwise film_interpolate calls on its float32 parents under the handle's current options.
 *   Cost.  Per primed push 2^T - 1 pair runs (flow estimator + fusion) and 2^(T - 1) feature extractions: the pushed frame's and one per
 *     fed-back mid-frame; the deepest mids are never extracted and no frame is extracted twice.  The runs go one after the other, one pair
 *     each (no breadth-first batching).  The stream plan holds T + 1 frame slots in its per-image buffers; if that workspace does not fit,
 *     film_stream_open returns FILM_ERR_NOMEM with "stream_times" in the message.  FILM_MEM_HOST: every frame is downloaded as soon as it
 *     is quantised, the call waits once at the end.
 *   film_stream_pair_plan_json  the plan of ONE pair run of a "stream_times" = `times` stream plan of `tiles` (padded) H x W tiles: image 0
 *                      is the frame in slot `left`, image 1 the one in slot `right` (slots 0 .. times: 0 and 1 take turns for the input
 *                      frames, slot 1 + d holds the depth-d mid-frame), and with extract != 0 the right frame's image pyramid and
 *                      extractor run first (ops [0, n_extract)), else "n_extract" is 0 and the plan holds no such op.  film_plan_json
 *                      text with "kind":"stream", "tiles", "slots" (= times + 1), "left", "right", "n_extract"; every orientation lists
 *                      the same buffers, whose per-image ones hold slots * tiles images.  times = 1, left = 1 - s, right = s, extract = 1
 *                      has the ops and buffers of film_stream_plan_json(slot = s).  FILM_ERR_INVALID: times outside 1 .. 6, left == right,
 *                      a slot outside 0 .. times.  Works on plan-only handles.
 *   film_stream_schedule_json  the pair runs of one primed push whose input frame lands in `slot` (0 / 1), in execution order:
 *                      {"times", "slot", "slots", "produced", "steps":[{"left", "right", "extract", "index", "depth", "feed"}, ...]} - the
 *                      step yields frame `index` (1 .. 2^T - 1) of `mid`, a depth-`depth` mid-frame, from the orientation (left, right,
 *                      extract), and cuts it into slot `feed` for its children (-1: it has none).  Works on plan-only handles.
 * Selected mid-frames (film_stream_select).  A frame-rate conversion that is no power of two wants a few of the 2^T - 1 positions of each
 * push, not all of them (film_hip/retime.py turns two rates into those choices).  A selection tells the open stream which ones:
 *   film_stream_select  bit i - 1 of `mask` stands for position i (1 .. 2^T - 1, temporal order) of the stream's "stream_times" = T.  The
 *                      selection belongs to the open stream: film_stream_open selects all 2^T - 1 positions, a selection holds for every
 *                      later push until it is changed, and film_stream_reset and a scene cut leave it as it is.  A primed push then writes
 *                      popcount(mask) frames to `mid`, packed in temporal order, and reports that count in *produced; every frame is
 *                      bit-identical to the frame at its position of a full push.  mask = 0 is allowed: such a push only extracts the
 *                      pushed frame, like a first push, reports *produced = 0 and takes a NULL `mid`.  FILM_ERR_STATE: no open stream.
 *                      FILM_ERR_INVALID, with "mask" in the message: a bit at or above 2^T - 1.
 *   What runs.  Let C be the selected positions and all their ancestors in the recursion (the parents a position is interpolated from, and
 *     theirs).  The push walks the depth-first order of film_stream_schedule_json restricted to C, one pair run per member.  A member with a
 *     child in C is fed back - cut as float32 into slot 1 + depth - as in a full push; a member that is not selected is joined (into the
 *     stream's own buffer) and fed back, but neither quantised nor downloaded nor written to `mid`.  In a full push a fed-back frame is
 *     extracted by its left child's run; when only the right child is in C, an extraction-only run stands in front of that child: the
 *     left child's orientation (its left slot, the fed-back frame's slot as `right`, extract = 1) run to "n_extract", as a first push runs
 *     its plan.  Per push: |C| pair runs, and 1 + (members of C with a child in C) extractions.  With every position selected the push
 *     makes exactly the device calls of a stream that was never given a selection.  The workspace, the T + 1 slots and the stream's
 *     buffers are those of 2^T - 1 frames whatever is selected.
 *   film_stream_select_schedule_json  the steps of the primed push of a "stream_times" = `times` stream with selection `mask` whose input
 *                      lands in `slot`: the keys of film_stream_schedule_json plus "mask"; "produced" = popcount(mask); every step gains
 *                      "deliver" (1: the frame goes to `mid`, 0: it is only fed back) and "run" ("pair", or "extract" for an
 *                      extraction-only step, whose "index" and "depth" are those of the frame it extracts, with "feed" -1 and "deliver"
 *                      0).  mask = 0: the one step is the extraction of the pushed frame ("index" 2^T, "depth" 0).  With the full mask
 *                      the steps are those of film_stream_schedule_json.  Refuses what that query refuses, and a bad mask as
 *                      film_stream_select does.  Works on plan-only handles.
 * Tile groups.  A stream whose T tiles do not fit one invocation runs every step of a push as G = ceil(T / n) runs of ONE stream plan of n
 * tiles, group after group; the last group holds the r <= n tiles that are left and runs the same plan (its surplus images compute on what
 * the group before left there; nobody reads them).  A device buffer of the stream's own, the CARRY, holds for every (group, frame slot) what a
 * pair run reads of an extracted frame: the per-image buffers of the plan that the ops of a pair run read and none of them writes (the
 * image and feature pyramids), one contiguous segment per buffer.  In front of a group's run the slots it reads are copied from the carry
 * into the plan, behind a run that extracted a frame that slot is copied out - one kernel launch each way (film_debug_segment_copy's).  Every
 * run is an ordinary run of an ordinary orientation, so every frame has the bits of the one-group stream and of film_interpolate.  The
 * order is outer = the steps of film_stream_select_schedule_json, inner = the groups: a frame that is fed back is the JOINED frame (cross-
 * faded with "block_overlap_*"), which exists when all groups of its step have run; it is then cut, group by group, into the carry.  The
 * carry is the truth about the carried frame: an evicted and rebuilt plan costs no re-extraction; a changed tile geometry re-extracts
 * every group from the stream's copy of the frame.  Options, selection, reset, scene cuts and duplicates mean what they mean for one group.
 * Memory: the workspace of n tiles plus (T + 1 slots) x (the pyramids of all tiles) of carry.
 *   film_stream_layout_json  the open stream: {"tiles", "groups", "group_tiles", "slots", "tile_h", "tile_w", "workspace_bytes",
 *                      "workspace_resident" (1: the plan of the groups holds its workspace on the device now, 0: it was evicted or dropped and the next
 *                      push allocates it again), "carry_bytes", "carry":[buffer names], "states":[{"group", "slot", "tile0", "ntiles", "segments":[{"buf", "plan_off",
 *                      "carry_off", "floats"}, ...]}, ...]} - offsets in floats into the plan's workspace and into the carry.  One group:
 *                      "groups" 1, "carry_bytes" 0, no carry buffers and no states.  FILM_ERR_STATE: no open stream.
 *   film_stream_group_schedule_json  the runs of the primed push of film_stream_select_schedule_json(times, slot, mask) for a frame of `tiles`
 *                      (padded) H x W tiles in groups of `group_tiles`: {"times", "slot", "slots", "mask", "produced", "tiles",
 *                      "group_tiles" (at most `tiles`), "groups", "carry":[buffer names], "steps":[...]}, one entry per step and group, in
 *                      execution order: the step's keys plus "step", "group", "tile0", "ntiles", "restore" (the slots copied whole from the
 *                      carry in front of the run), "cut" (where the extracted frame comes from: "keep" - cut from the stream's copy of the
 *                      pushed frame; "carry" - the img0 tiles its parent's feed-cut left in the carry are restored; "plan" - one group: they
 *                      are in the plan; "none": nothing is extracted), "save" (the slot copied whole into the carry behind the run, -1:
 *                      none), "join" ([tile0, ntiles] of a pair run, else []), "last" (1: the step's last group - its frame is delivered)
 *                      and "feed_to" ("carry" / "plan": behind the last group the frame is cut into slot "feed" there; "none").  One group:
 *                      the steps of film_stream_select_schedule_json with no restore and no save.  A first push is mask = 0.  Refuses what
 *                      that query refuses and tiles or group_tiles < 1.  Works on plan-only handles. */
#define FILM_PIX_F32 0   /* frames and results float32 [H,W,3], as everywhere else */
#define FILM_PIX_U8  1   /* frames and results uint8 [H,W,3]: x = u8 / 255.0f (IEEE, = read_image), result = film_to_uint8's rule */
/* 8-bit Y'CbCr 4:2:0 frames: the conversion in is fused into the tile cut, the conversion out into the quantisation, so such a frame
 * crosses PCIe as 1.5 bytes per pixel each way and the caller needs no colour kernels of its own.  `pix` = a layout in bits 0-7 plus
 * colour flags.  FILM_ERR_INVALID, with "pix" in the message: any other bit set; a colour flag together with FILM_PIX_F32 / FILM_PIX_U8;
 * an odd H or W with a 4:2:0 layout (4:2:0 needs even sizes).  Device pointers to 4:2:0 frames must be 4-byte aligned (as for
 * FILM_PIX_U8: the cut reads the aligned 32-bit words that hold a row's bytes, none of which lies outside the allocation rounded up to
 * whole words). */
#define FILM_PIX_I420   16      /* Y[H][W], Cb[H/2][W/2], Cr[H/2][W/2], contiguous: H*W*3/2 bytes */
#define FILM_PIX_NV12   17      /* Y[H][W], CbCr[H/2][W/2][2] interleaved: H*W*3/2 bytes */
/* 10-bit Y'CbCr 4:2:0 frames: the same planes with one little-endian uint16 per sample, H * W * 3 bytes a frame - what a hardware decoder hands over
 * for HEVC Main10, AV1 and VP9 profile 2 (P010) and what `ffmpeg -pix_fmt yuv420p10le` pipes (I010).  Same flags, same refusals (even sizes; any other bit;
 * device pointers 4-byte aligned); fused into the cut and the quantisation like the 8-bit layouts ("The 10-bit 4:2:0 arithmetic" below).  The transfer
 * function (PQ, HLG, gamma) is not the engine's business: the network sees the non-linear samples it was given. */
#define FILM_PIX_I010   32      /* Y[H][W], Cb[H/2][W/2], Cr[H/2][W/2], little-endian uint16, code in bits 0-9 (= yuv420p10le, Y4M C420p10): H*W*3 bytes */
#define FILM_PIX_P010   33      /* Y[H][W], CbCr[H/2][W/2][2], little-endian uint16, code in bits 6-15 (what VCN / VA-API / D3D decoders emit): H*W*3 bytes */
/* Planar Y'CbCr 4:2:2 and 4:4:4 frames, 8-bit and 10-bit: mezzanine / broadcast video (4:2:2, mostly 10-bit), screen captures, animation masters and
 * graphics (4:4:4).  Same flags, same fusion into the cut and the quantisation ("The 4:2:2 and 4:4:4 arithmetic" below).  S = the samples of a frame:
 * 2 H W (4:2:2) or 3 H W (4:4:4).  4:2:2 needs an even W (an odd H is fine; the message contains "4:2:2 needs an even width"); 4:4:4 takes any
 * H, W >= 1, like the RGB layouts.  Device pointers stay 4-byte aligned (2-byte for a 10-bit dst of the quantiser), inside an allocation of whole
 * 32-bit words; in a batch (film_debug_yuv_cut, B > 1) frame b starts at sample b * S, which for an odd-sized 4:4:4 frame is no word boundary: the
 * kernels read the aligned words that hold a sample. */
#define FILM_PIX_I422   20      /* Y[H][W], Cb[H][W/2], Cr[H][W/2], bytes (= yuv422p, Y4M C422): 2*H*W bytes */
#define FILM_PIX_I444   24      /* Y[H][W], Cb[H][W], Cr[H][W], bytes (= yuv444p, Y4M C444): 3*H*W bytes */
#define FILM_PIX_I210   36      /* as I422, little-endian uint16, code in bits 0-9 (= yuv422p10le, Y4M C422p10): 4*H*W bytes */
#define FILM_PIX_I410   40      /* as I444, little-endian uint16, code in bits 0-9 (= yuv444p10le, Y4M C444p10): 6*H*W bytes */
#define FILM_YUV_BT601  0x100   /* matrix: absent = BT.709 */
#define FILM_YUV_FULL   0x400   /* range: absent = limited (8-bit 16..235 / 16..240, 10-bit 64..940 / 64..960) */
#define FILM_YUV_BT2020 0x2000  /* matrix: BT.2020 non-constant luminance, (Kr, Kb) = (0.2627, 0.0593) - what nearly all 10-bit UHD / HDR content is coded with.
                                 * Valid with every Y'CbCr layout and with FILM_YUV_FULL; together with FILM_YUV_BT601: FILM_ERR_INVALID ("pix" in the
                                 * message).  Constant-luminance BT.2020 and the transfer function (PQ, HLG) stay the caller's business. */
/* The 4:2:0 arithmetic.  Every operation is float32 with one rounding, no fused multiply-add.  (Kr, Kb) = (0.2126, 0.0722) for BT.709,
 * (0.299, 0.114) for BT.601, (0.2627, 0.0593) for BT.2020 (FILM_YUV_BT2020), Kg = 1 - Kr - Kb; every constant below is computed from them in double and rounded to float32 once.
 *   In (bytes -> RGB).  Per-byte tables, IEEE division on the host: limited range y[v] = (float(v) - 16) / 219, c[v] = (float(v) - 128) / 224;
 *     full range y[v] = float(v) / 255, c[v] = (float(v) - 128) / 255.  Pixel (y, x) takes the chroma sample (y >> 1, x >> 1): chroma is
 *     treated as centre-sited and replicated.  With y = y[Y], cb = c[Cb], cr = c[Cr]:
 *       R = y + a_r * cr              a_r = 2 (1 - Kr)
 *       B = y + a_b * cb              a_b = 2 (1 - Kb)
 *       G = (y - g_b * cb) - g_r * cr     g_b = 2 Kb (1 - Kb) / Kg, g_r = 2 Kr (1 - Kr) / Kg
 *     each then clipped: max(., 0) followed by min(., 1).
 *   Out (RGB -> bytes).  Per channel x = min(max(v, 0), 1) (write_image's clip), then
 *       Yf  = (kr * R + kg * G) + kb * B              kr, kg, kb = float32(Kr), float32(Kg), float32(Kb)
 *       cbf = (B - Yf) * s_b          s_b = 0.5 / (1 - Kb)
 *       crf = (R - Yf) * s_r          s_r = 0.5 / (1 - Kr)
 *     chroma of the 2 x 2 block (j, k): m = ((c[2j][2k] + c[2j][2k+1]) + (c[2j+1][2k] + c[2j+1][2k+1])) * 0.25
 *     q(v) = uint8(min(max(v, 0), 255) + 0.5);  limited: Y = q(Yf * 219 + 16), C = q(m * 224 + 128);  full: Y = q(Yf * 255), C = q(m * 255 + 128).
 *   Replicate in and box mean out are inverse to each other: a frame whose RGB stays inside the gamut returns byte for byte.
 * The 10-bit 4:2:0 arithmetic (FILM_PIX_I010 / FILM_PIX_P010).  The matrix constants, the operation order, the replicated chroma in, the 2 x 2 box
 * mean out in the same summation order and the places of the clips are those of the 8-bit arithmetic above; every operation is float32 with one
 * rounding, no fused multiply-add.  Only the codes change.
 *   Code of a stored word w.  I010: v = w & 1023 (the upper six bits are ignored).  P010: v = w >> 6 (the lower six bits are ignored).  0 <= v <= 1023
 *     for every word.
 *   In (words -> RGB).  IEEE float32 division: limited range y[v] = (float(v) - 64) / 876, c[v] = (float(v) - 512) / 896; full range
 *     y[v] = float(v) / 1023, c[v] = (float(v) - 512) / 1023.  Then R, G, B as above.
 *   Out (RGB -> words).  Yf, cbf, crf and m as above; q10(x) = uint16(min(max(x, 0), 1023) + 0.5);  limited: Y = q10(Yf * 876 + 64),
 *     C = q10(m * 896 + 512);  full: Y = q10(Yf * 1023), C = q10(m * 1023 + 512).  I010 stores the code, P010 stores code << 6: the ignored bits
 *     are written as zero.
 *   A frame whose decoded RGB stays inside the gamut returns code for code (tests/test_yuv10_cpu.py checks it for all four colour settings).
 * The 4:2:2 and 4:4:4 arithmetic (FILM_PIX_I422 / I444: the 8-bit arithmetic; FILM_PIX_I210 / I410: the 10-bit one, code v = w & 1023).  Constants,
 * operation order, clips, code rules, ranges and quantisers are those of the two sections above.  Only the chroma pairing and the mean change.
 *   In.   4:2:2: pixel (y, x) takes the chroma sample (y, x >> 1).  4:4:4: pixel (y, x) takes the chroma sample (y, x).  As in 4:2:0 the pairing
 *     follows the frame coordinate, not the tile's.
 *   Out.  4:2:2: m = (c[y][2k] + c[y][2k+1]) * 0.5f.  4:4:4: m = c[y][x], no mean.
 *   A frame whose decoded RGB stays inside the gamut returns code for code (tests/test_yuv_chroma_cpu.py checks it for both depths, the three
 *   subsamplings and all six colour settings).
 *   Not provided (at any depth): 12-bit and deeper samples; semi-planar or packed 4:2:2 / 4:4:4 (NV16, P210, NV24, v210, Y410); constant-luminance
 *   BT.2020 (flag bits 0x200 / 0x800 / 0x1000 and every other bit stay refused); sited bilinear chroma (MPEG-2 left siting - the box treatment is
 *   consistent in and out); Y'CbCr frames on film_interpolate / film_interpolate_sequence themselves (film_to_yuv converts their results).
 * Scene cuts.  Across a cut a stream would interpolate between two unrelated pictures.  The engine offers an exact per-frame statistic
 * computed where the frame already lies, an integer decision rule, and a stream that resets itself (option "scene_cut").  Integers only.
 *   Histogram of a frame: uint32_t hist[3][256], hist[p][v] = the number of samples of plane p with 8-bit code v.
 *     FILM_PIX_U8     plane c = the bytes frame[y][x][c].
 *     FILM_PIX_F32    plane c = the byte film_to_uint8 stores for frame[y][x][c]: uint8(clip(x * 255, 0, 255) + 0.5), the same float32
 *                     operations in the same order.
 *     FILM_PIX_I420 / FILM_PIX_NV12   plane 0 = the Y bytes (H * W samples), planes 1 and 2 = the Cb and Cr bytes (H/2 * W/2 samples each).
 *                     The colour flags are validated as everywhere else and otherwise ignored: the statistic is about the stored codes.
 *     FILM_PIX_I010 / FILM_PIX_P010   the same planes and sample counts; a sample with 10-bit code v counts in bin v >> 2, so the [3][256]
 *                     layout, S and the rule below do not change.
 *     FILM_PIX_I422 / I444 / I210 / I410   plane 0 = the H * W Y samples, planes 1 and 2 = the Cb and Cr samples: H * W / 2 each (4:2:2) or H * W each
 *                     (4:4:4); a 10-bit sample counts in bin code >> 2.
 *     Every plane sums to its sample count.  S = the samples of one frame: 3 H W for RGB and 4:4:4, 3 H W / 2 for 4:2:0, 2 H W for 4:2:2.
 *   Distance: D = sum over p, v of |h1[p][v] - h0[p][v]|, an int64 with 0 <= D <= 2 S; the score is D / (2 S).  Moving content leaves it
 *     at 0 (a permutation of the samples has the same histogram); two frames with no code in common give 1.
 *   Rule: with "scene_cut" = k, 1 <= k <= 1000 (permille), a pair of frames is a cut iff 1000 D >= k * 2 S, compared in 64-bit integers.
 *     k = 0 (default) turns the feature off.
 *   NO default threshold is recommended: the detector's hit and miss rates on real footage are UNMEASURED (no footage was available when
 *   this was written) - choose k on your own material.  What a global histogram cannot see: two scenes with alike histograms (a cut
 *   between them is missed); fades and dissolves (every step is small); flashes (one bright frame reads as two cuts).
 *   film_frame_histogram: the histogram of ONE H x W frame of pixel type `pix`, like film_to_uint8 / film_to_yuv420 on DEVICE pointers and
 *     without a handle: asynchronous on `stream` (NULL: the default stream) of the current device.  hist_dev receives 768 uint32_t
 *     ([3][256]); the call overwrites them - it never accumulates.  frame_dev must be 4-byte aligned and, for the 8-bit types, lie in an
 *     allocation of whole 32-bit words (as for the 8-bit cuts: the last partial word is read, only the frame's bytes are counted; a 10-bit frame is
 *     whole words).
 *     FILM_ERR_INVALID: a NULL pointer, H or W < 1, H * W >= 2^31, a pix the stream entry points refuse (odd sizes with 4:2:0 included),
 *     a frame_dev that is not 4-byte aligned.
 * Duplicate frames.  Film in a 30p or 60p container, animation drawn on twos and threes, screen captures and anything converted from a variable
 * to a constant frame rate repeat frames; interpolating between two copies of one picture costs a full push and keeps the stutter.  The histogram
 * above cannot see a repeat (its distance is 0 for pure motion too).  The engine offers an exact, spatially aware statistic of two frames, an
 * integer decision rule, and a stream that ignores a push judged a duplicate (options "dup_hi", "dup_lo", "dup_frac").  Integers only.
 *   Planes and codes.  Two frames a, b of one `pix`, H and W.  The planes and their sizes are those of the histogram: plane 0 is H x W, planes 1
 *     and 2 are (H >> sy) x (W >> sx) for Y'CbCr - (sx, sy) = (1, 1) for 4:2:0, (1, 0) for 4:2:2, (0, 0) for 4:4:4 - and H x W for the RGB types; the
 *     Cb and Cr planes of FILM_PIX_NV12 / P010 are the de-interleaved samples.  The code of a sample is taken at FULL depth: the stored byte (8-bit
 *     layouts); w & 1023 (FILM_PIX_I010 / I210 / I410); w >> 6 (FILM_PIX_P010); the byte frame[y][x][c] (FILM_PIX_U8); the byte film_to_uint8
 *     stores for frame[y][x][c], by the float32 operations of the FILM_PIX_F32 histogram (FILM_PIX_F32).
 *   Blocks.  Block (i, j) of a plane of Hp x Wp samples holds rows 8 i .. min(8 i + 8, Hp) - 1 and columns 8 j .. min(8 j + 8, Wp) - 1: the grid is
 *     anchored on the plane, partial blocks at the right and bottom edge count as they are, blocks_p = ceil(Hp / 8) * ceil(Wp / 8).  The SAD of a
 *     block is s = sum |a - b| over its samples, at most 64 * 1023 = 65472.
 *   Result: uint64_t out[3][4], out[p] = {total, max, over, blocks} of plane p: total = the sum of s over its blocks (past 2^32 at 4K, hence 64
 *     bits), max = the largest s, over = the number of blocks with s > lo (strictly; `lo` is a call argument in stored-code units), blocks = blocks_p.
 *   Rule: with "dup_hi" = h >= 0, "dup_lo" = l and "dup_frac" = f, and m = 1 for the 8-bit, U8 and F32 types and m = 4 for the 10-bit layouts (a
 *     value then means the same on the 8- and 10-bit versions of one video, as code >> 2 does for the histogram), frame b is a duplicate of
 *     frame a iff for EVERY plane p: max_p <= h * m and 1000 * over_p <= f * blocks_p, with over counted at lo = l * m; all in 64-bit integers.
 *     h = 0 with the other defaults (l = 0, f = 1000) means exact duplicates only.
 *   NO values are recommended: hit and miss rates on real footage are UNMEASURED, as for "scene_cut" - choose them on your own material.  (The
 *   defaults of ffmpeg's mpdecimate filter, hi = 768, lo = 320, frac = 0.33, are that filter's own, for a different block definition; they are
 *   named here for orientation and not endorsed.)
 *   film_frame_diff: the statistic of TWO H x W frames of pixel type `pix` on DEVICE pointers, without a handle, asynchronous on `stream`
 *     (NULL: the default stream) of the current device, like film_frame_histogram.  out_dev receives the 12 uint64_t; the call overwrites them -
 *     it never accumulates.  Alignment and allocation contract of a_dev and b_dev: film_frame_histogram's.  The colour flags are validated and
 *     otherwise ignored: the statistic is about the stored codes.
 *     FILM_ERR_INVALID: what film_frame_histogram refuses (a NULL pointer, H or W < 1, H * W >= 2^31, a pix the stream entry points refuse, a frame
 *     pointer that is not 4-byte aligned), lo outside 0 .. 65535, an out_dev that is not 8-byte aligned.
 *   film_stream_dup_info: what the last push found with option "dup_hi" >= 0: stats[12] = the out[3][4] of its comparison, or twelve -1 when
 *     none was made (the option is -1, the first frame, the push after a reset or a failed push); *dup = 1 when the push was dropped as a
 *     duplicate, else 0.  NULL outputs are skipped.  FILM_ERR_STATE: no open stream. */
int film_frame_histogram(const void* frame_dev, int H, int W, int pix, uint32_t* hist_dev, void* stream);
int film_stream_cut_info(film_t* h, int64_t* distance, int64_t* samples, int* cut);
int film_frame_diff(const void* a_dev, const void* b_dev, int H, int W, int pix, int lo, uint64_t* out_dev, void* stream);
int film_stream_dup_info(film_t* h, int64_t stats[12], int* dup);
int film_stream_open(film_t* h, int H, int W, int align, int block_h, int block_w, int pix);
int film_stream_push(film_t* h, const void* frame, void* mid, int* produced, int mem_kind, void* stream);
int film_stream_reset(film_t* h);
int film_stream_close(film_t* h);
int film_stream_plan_json(film_t* h, int tiles, int H, int W, int slot, char* buf, int64_t capacity, int64_t* needed);
int film_stream_pair_plan_json(film_t* h, int tiles, int H, int W, int times, int left, int right, int extract, char* buf, int64_t capacity,
                               int64_t* needed);
int film_stream_schedule_json(film_t* h, int times, int slot, char* buf, int64_t capacity, int64_t* needed);
int film_stream_select(film_t* h, uint64_t mask);
int film_stream_select_schedule_json(film_t* h, int times, int slot, uint64_t mask, char* buf, int64_t capacity, int64_t* needed);
int film_stream_layout_json(film_t* h, char* buf, int64_t capacity, int64_t* needed);
int film_stream_group_schedule_json(film_t* h, int tiles, int H, int W, int times, int slot, uint64_t mask, int group_tiles, char* buf,
                                    int64_t capacity, int64_t* needed);

/* Execution options.  Keys:
 *   "autotune" 0/1 time every distinct conv shape of a new plan with each fitting tile shape and keep
 *                  the fastest (default 1; cannot change results - same k-ordered fma chain per output)
 *   "graph"   0/1/2  how a plan's ops reach the device.  2 (default): direct launches on two lanes - lane 0 on the caller's
 *                  stream, lane 1 (small subtrees, coarse flow levels, the t = 0.5 warps) on a side stream of the handle, ordered by
 *                  events; 1: the same two lanes captured once per (B, H, W) into a hipGraph and replayed; 0: one stream, plan order.
 *                  Identical results.  The graph is opt-in since round 5: the HIP 7.0 runtime PyTorch 2.10 bundles can crash in the
 *                  first launch of a fresh multi-branch graph late in a long-lived process (profiles/r05_hipgraph_first_launch_crash.md)
 *   "profile" 0/1  record a hipEvent pair around every kernel of the next forwards
 *                  (forces graph off); read the result with film_profile_json
 *   (options marked [extra] exist only in a library built with FILM_EXTRA_FAMILIES=1 - libfilm_hip_extra.so, see film_version();
 *   the default library, which holds only the kernel families a default plan can select, refuses them with a message)
 *   "precision" p  [extra for 1, 2]  0 (default): every convolution on the exact fp32 MFMA.  1: "bf16x6" - the large 3x3
 *                  convolutions split each fp32 operand exactly into three bf16 pieces and accumulate the six
 *                  partial products >= 2^-16 in fp32 on the bf16 matrix pipe (dropped terms < 2^-23 relative);
 *                  about 1.5x faster, results differ from mode 0 at the level of a changed summation order.
 *                  2: "bf16x3" - the same kernels with a nearest 2-way split (hi + mid, |x - hi - mid| <= 2^-17 |x|)
 *                  and the three products hi*hi + hi*mid + mid*hi: per-product error <= 2^-15 relative in the worst
 *                  case, 4.4e-6 rms, zero mean (not an fp32 result; 7e-6 from the oracle end to end against the 1e-3
 *                  image bound, see tests).
 *                  Changing it drops the cached plans.
 *   "lanes"   0/1/2  >= 1 (default 1): replay graphs run the independent small / HBM-bound kernels (feature subtrees of the coarse
 *                  pyramid levels, coarse flow levels, the t = 0.5 warps) on a second stream beside the main chain;
 *                  2 (measured 2 % slower at 1080p, not the default): on frames larger than 512 x 512 the coarse decoder levels (>= 2) join that stream right behind
 *                  the aligned levels they read, so that their matrix-bound convolutions run beside the flow estimator's
 *                  chain of HBM-bound warps and short launches instead of behind it.  Ordering between the two streams
 *                  comes from a buffer-overlap analysis of the plan.  3 = the same on frames of any size (tests).  Drops the
 *                  cached plans.
 *   "splitk"  0/1  1 (default): the deep convolutions of pyramid levels with <= 4096 pixels per image run split-K
 *                  (2-16 partial sums over K ranges, added in split order by a second kernel: deterministic, and the
 *                  factor depends on the level size and the layer only, never on the batch); it is what bounds the
 *                  latency of small frames.  Changing it drops the cached plans.
 *   "pack_groups" n  pack (and upload) the first n of the four weight layout groups now (normally packed on demand; the groups:
 *                  kLayouts in csrc/film_layers.cpp)
 *   "fuse"    bits 31 (default): small-launch fusion, identical arithmetic and bit-identical results.  1: tf.image.resize(2 * v)
 *                  of the flow estimator inside the warp kernels that consume it; 2: v = residual + upsampled flow inside
 *                  the flow-head kernels; 4: the warped images and the half flows of the t = 0.5 stage (the sixteen miscellaneous
 *                  channels of an aligned level) inside the second feature warp of the level; 8: AveragePooling2D of the sub-extractor
 *                  stages in the epilogue of the F(4,3) convolution in front of it (about 35 launches fewer per forward in all);
 *                  16: the RGB head (1x1 convolution, fusion.py:138-140) in the epilogue of the last decoder layer, whose
 *                  64-channel output is then never written.  0: one launch per reference op.  Drops the cached plans.
 *   "fold2x2" 0-2  the decoder's nearest-x2 upsample + 2x2 convolution (fusion.py:133-135) on the LOW-resolution input.
 *                  1 (default): in its difference form - four products per low-resolution pixel (with I, Dx = I - I(x+1),
 *                  Dy = I - I(y+1), Dxy and the weight sums S, Sx, Sy, W11: out(2y+py, 2x+px) = S.I - px Sx.Dx - py Sy.Dy +
 *                  py px W11.Dxy), conv_fold4_kernel; 2: as four sub-pixel phase convolutions with pre-summed weights (9 taps
 *                  per 4 outputs instead of 16; the general kernel).  Both are exact regroupings of the sum, the rounding
 *                  differs at the 1e-7 level.  0: one 2x2 convolution with the upsample folded into its gather.
 *                  Drops the cached plans.
 *   "planar" 0/1   1 (default): an aligned-pyramid level (interpolator.py:167-183) is stored as three pixel-major planes -
 *                  warp(features of image 0), warp(features of image 1), the sixteen image / flow channels - each written
 *                  contiguously by its warp, and read by the decoder as three input segments in the reference's channel
 *                  order (same weights, same sums, same bits); film_get_tap("aligned<l>") interleaves them.  0: one
 *                  [N][H][W][2C + 16] buffer per level.  Drops the cached plans.
 *   "winograd" w   1 (default): the large 3x3 convolutions use a 1-D Winograd transform along x - F(4,3) (2x fewer
 *                  fp32 multiplies, 128-pixel patches) on the levels whose width fills its patches, F(2,3) (1.5x fewer)
 *                  elsewhere; fp32 throughout, the rounding differs from the direct sum at the 1e-6 (F(2,3)) /
 *                  5e-6 (F(4,3)) level.  0: direct kernels only.  2 [extra] / 3: F(2,3) / F(4,3) on every eligible 3x3
 *                  convolution (tests).  Changing it drops the cached plans.
 *   "halo_all" 0/1 [extra] run every eligible 3x3 convolution on the halo-staged kernels whatever its size (default 0:
 *                  only where measured faster); "tune_ms" n: autotune spends at least n ms per candidate.
 *                  Test / tuning knobs; "halo_all" drops the cached plans.
 *   "wino2d"  0/1/2  1 (default): every 3x3 convolution whose channels come in sixteens, on levels of >= "w2d_min_px" (1536) pixels per image
 *                  - and on smaller ones down to "w2d_small_px" (256) pixels that fill >= 65 % of their 8-row x 32-pixel tiles - runs the nested
 *                  Winograd form F(4,3) along x times F(2,3) along y (conv_wino2d_kernel: 3 multiplies per output where the 1-D
 *                  F(4,3) kernel spends 4.5 and the direct convolution 9; fp32 throughout, rounding at the level of the 1-D form).
 *                  0: never.  2: every layer that has the weight copy, on every level (tests).  Drops the cached plans.
 *   "w2d_min_px" n / "w2d_small_px" n  the two level-size thresholds of that rule (A/B runs; a function of the level only - never the batch).
 *   "w2d_splitk" 0/1/2..16  1 (default): the nested kernel's K >= 768 layers on levels of <= 4096 pixels per image (the 36x60 level of a 1080p
 *                  tile, the 64x64 level of a 256x256 pair) run as up to four K ranges + the ordered reduction, like "splitk"
 *                  (which also switches it off); factor from the level size and the layer only.  0: never.  n = 2..16 (A/B runs): the
 *                  same, and the K >= 384 layers on levels of <= 1024 pixels run as up to n K ranges (min(n, K / 192)).  Drops the cached plans.
 *   "w43_shape" n  test knob: every convolution on conv_wino43_kernel that can run tile shape n (Wino43Tile, film_kernels.h)
 *                  does, instead of the autotuned shape; -1 (default) = autotuned.  Results cannot change.  Drops the cached plans.
 *   "w2d_shape" n  the same for conv_wino2d_kernel (Wino2dTile: 0..2 = 8 rows x 32 pixels, 3..5 = 16 x 16 pixels - the latter only on levels it pads no more).
 *   "fold4_shape" n  the same for conv_fold4_kernel (Fold4Tile).
 *   "max_batch" n  process at most n frame pairs / tiles per model invocation (0 = only the built-in limits: 64 GiB of
 *                  workspace, 4 GiB per buffer read through a whole-buffer 32-bit offset); frame pairs are independent,
 *                  results do not change
 *   "host_overlap" 0/1  1 (default): film_interpolate with FILM_MEM_HOST pipelines its copies with the work - the second frame is uploaded
 *                  while the first layers run on the first frame's tiles, the upper half of the result is downloaded while the last layer
 *                  computes the lower half (one frame, an even number of block rows); 0: upload, work, download.  Same bits.
 *                  (film_interpolate only: film_interpolate_sequence and film_stream_push always upload, work, download.)
 *                  (Not taken with overlapped tiles, whose upper half depends on the lower tiles: upload, work, download.)
 *   "block_overlap_h" o / "block_overlap_w" o  (extension; -1 .. 65535, default 0 = the reference's disjoint patches, today's kernels)
 *                  the tiled path of film_interpolate / film_interpolate_sequence / film_stream_push, per axis of nb blocks of p = n / nb pixels:
 *                  every tile takes o pixels of its neighbours on both sides and the tiles' results are cross-faded over the
 *                  shared pixels, so that no step is left along the patch borders.  nb == 1: no overlap.  -1 ("free"):
 *                  o = min(pad0 / 2, p / 2), pad0 = the zero padding `align` gives a p-sized patch - the padded tile and the
 *                  plan stay the same.  Otherwise 2 o <= p, else the compute calls and film_tiling_json return FILM_ERR_INVALID.
 *                  Tile i holds the e = p + 2 o pixels from s_i = clamp(i p - o, 0, n - e) (tiles at the frame's edge reach 2 o
 *                  inwards), padded to `align` like a patch.  Weight of tile i at position y inside it: a_i(y) = the distance to
 *                  its nearest interior edge (y - s_i + 1, s_i + e - y; an edge on the frame's border does not limit it),
 *                  normalised in float32, w_i(y) = a_i(y) / sum_i a_i(y).  A pixel = sum over the covering tiles (i, j) in
 *                  row-major order of (wy_i * wx_j) * value, float32, one rounding per operation, no fused multiply-add;
 *                  independent of how the tiles are chunked.  Does not drop the cached plans (their key carries the tile size).
 *   "stream_times" T  (extension; 1 .. 6, default 1 = today's streams: the same plan, device calls, workspace and bits)  read by
 *                  film_stream_open and fixed for that stream's life - a later change affects the next open only.  T > 1: a primed
 *                  film_stream_push writes 2^T - 1 frames ("Recursive mid-frames" above).  Does not drop the cached plans (their key
 *                  carries the slot count).
 *   "scene_cut" k  (extension; 0 .. 1000 permille, default 0 = off, today's pushes: no launch, copy, allocation or wait is added)  read at
 *                  every film_stream_push, like "block_overlap_*".  k > 0: after the frame has reached the stream's own copy the push
 *                  takes its histogram there (film_frame_histogram's kernel), downloads the 3 KB and WAITS for them - so also a
 *                  device-resident push blocks the calling thread until the histogram is back - and compares it with the previous
 *                  frame's ("Scene cuts" above: cut iff 1000 D >= k * 2 S).  No cut: the push goes on as always.  Cut: the push behaves
 *                  exactly as film_stream_reset followed by this push - *produced = 0, `mid` is not touched, only the extraction runs
 *                  (no flow estimator, no fusion) - and the next push interpolates inside the new scene.  No comparison is made on the
 *                  first frame, after film_stream_reset, after a failed push, and on the first push after the option was turned on.
 *                  film_stream_cut_info reports what the last push found.  No threshold is recommended: see "Scene cuts".  Does not
 *                  drop the cached plans.
 *   "dup_hi" h / "dup_lo" l / "dup_frac" f  (extension; h: -1 .. 16320, default -1 = off, today's pushes: the frame is copied straight into the
 *                  stream's copy and no launch, copy, allocation or wait is added; l: 0 .. 16320, default 0; f: 0 .. 1000 permille, default
 *                  1000)  read at every film_stream_push.  h >= 0: the pushed frame is uploaded or copied into a SECOND keep buffer of the
 *                  stream (allocated by the first such push).  On a primed stream film_frame_diff's kernel compares it there with the carried
 *                  frame's copy, the 96 bytes are downloaded and WAITED for - so also a device-resident push blocks the calling thread - and
 *                  the rule of "Duplicate frames" above decides.  Duplicate: the push ends there with *produced = 0; `mid` is untouched and
 *                  the stream is exactly as before the call - primed state, slot, carried frame and its copy, carried histogram, selection and
 *                  plan; no cut, extraction or pair run is queued, no histogram is taken, and film_stream_cut_info reports that no comparison
 *                  was made (-1, cut 0).  Not a duplicate: the two keep buffers swap roles and the push goes on as always, the "scene_cut"
 *                  histogram of the new frame included: duplicates are decided first and never count as cuts.  The carried frame of a run
 *                  of near-duplicates is the FIRST of the run and every later frame is compared with it, the last kept one, so slow drift
 *                  is eventually seen.  No comparison is made on an unprimed push (the first, after film_stream_reset, after a failed push).
 *                  The argument checks of a push come first, a NULL `mid` on a primed push included; a failure behind them unprimes the
 *                  stream as always.  film_stream_dup_info reports what the last push found.  No values are recommended: see "Duplicate
 *                  frames".  None of the three drops the cached plans. */
int film_set_option(film_t* h, const char* key, int64_t value);

/* The tile geometry film_interpolate / film_interpolate_sequence use for H x W frames with these arguments and the handle's current
 * "block_overlap_h" / "block_overlap_w" as JSON (buf / capacity / needed as film_plan_json; works on plan-only handles):
 * "overlap_h", "overlap_w" (resolved), "tile_h", "tile_w" (tile content), "padded_h", "padded_w" (the H x W of the plan),
 * "pad_y", "pad_x" (content offset inside the padded tile), "origins_y", "origins_x" (first frame row / column of every tile row /
 * column).  Same refusals as the compute calls (block divisibility, overlap larger than half a patch). */
int film_tiling_json(film_t* h, int H, int W, int align, int block_h, int block_w, char* buf, int64_t capacity, int64_t* needed);

/* Autotune choices across processes.  film_export_tune writes text (buf / capacity / needed as film_plan_json): a header
 * line with the library version, then "<conv shape signature>\t<tile id>" per shape this handle measured or imported.
 * film_import_tune takes such text before the first forward: shapes found in it are not measured again (first call of a
 * 1080p plan 2.5 s -> the plan build + graph capture alone).  Text from another library version is ignored, entries are
 * validated against the kernel family of the op that wants them, and results never depend on the cache (every tile of a
 * family produces the same bits).  film_hip.engine reads / writes the file named by $FILM_TUNE_CACHE with these. */
int film_export_tune(film_t* h, char* buf, int64_t capacity, int64_t* needed);
int film_import_tune(film_t* h, const char* text);

/* Per-kernel-class timing of the last profiled forward as JSON
 * {"classes": {"conv_mfma": {"launches": n, "ms": t, "flops": f, "bytes": b}, ...}}. */
int film_profile_json(film_t* h, char* buf, int64_t capacity, int64_t* needed);

/* Description of the plan for (B,H,W) as JSON: named workspace buffers (offset, dims),
 * the op list with every kernel parameter and the packed-weight offsets.  Works on
 * plan-only handles; tests interpret it against a numpy arena to validate planner and
 * weight packing without a GPU.  "offset32_buffer_bytes" = the largest buffer a kernel with whole-buffer 32-bit
 * offsets reads (must stay below 4 GiB; conv_wino43_kernel and the pointer-addressed kernels are not limited). */
int film_plan_json(film_t* h, int B, int H, int W, char* buf, int64_t capacity, int64_t* needed);

/* The same for the sequence plan of n_pairs consecutive frame pairs of tiles_per_frame (padded) H x W tiles each, as
 * film_interpolate_sequence runs it: "kind":"sequence", "n_pairs", "tiles"; B = n_pairs * tiles_per_frame pair-tiles; img0 holds
 * (n_pairs + 1) * tiles_per_frame images, frame-major (pair-tile p reads images p and p + tiles_per_frame).  Works on plan-only handles. */
int film_sequence_plan_json(film_t* h, int n_pairs, int tiles_per_frame, int H, int W, char* buf, int64_t capacity,
                            int64_t* needed);

/* Copies a named workspace buffer of the last forward (see "buffers" in film_plan_json) to a
 * host array; dims receives {N,H,W,C}.  Debug / parity taps, mirrors the aux outputs of
 * models/film_net/interpolator.py:191-199. */
int film_get_tap(film_t* h, const char* name, float* dst, int64_t capacity_floats, int64_t dims[4]);

/* Debug / tests: ONE planned kernel launch on a workspace the caller controls (tests/op_harness.py, tests/test_ops_gpu.py).  Both take
 * the plan key (B, H, W, tiles): tiles = 0 for the plan of film_forward / film_interpolate, > 0 for the sequence plan of B / tiles pairs
 * of `tiles` tiles (film_sequence_plan_json).  Both create the device plan as a forward would (workspace, autotune when the option is
 * on) and make it the plan film_get_tap reads.  FILM_ERR_NO_DEVICE on plan-only handles, FILM_ERR_STATE before film_finalize.
 * Neither is on the forward path.
 * film_debug_arena: copies `count` floats at float offset `offset` of that plan's workspace ("arena_floats" and every "off" of
 * film_plan_json) to the host array `data` (write == 0) or from it (write != 0), after the handle's stream has drained.
 * FILM_ERR_INVALID when the range leaves the workspace. */
int film_debug_arena(film_t* h, int B, int H, int W, int tiles, int64_t offset, int64_t count, float* data, int write);
/* film_debug_run_op: launches op `index` ("ops" of film_plan_json) of that plan once on the handle's stream and synchronises.
 * candidate == -1 runs the tile the plan holds; candidate == k >= 0 runs entry k of the autotune candidate list of the op's kernel
 * family for this op - the only way to choose a tile, so a shape the family's own rule excludes cannot be launched.  *n_candidates
 * (may be NULL) receives the length of that list: 0 for an op that is no convolution, which accepts -1 only.  FILM_ERR_INVALID: no
 * such op, no such candidate. */
int film_debug_run_op(film_t* h, int B, int H, int W, int tiles, int index, int candidate, int* n_candidates);
/* film_debug_tile_map: ONE cut (mode 0: frames -> tiles) or ONE join (mode 1: tiles -> frames) of tiles [tile0, tile0 + ntiles) of a batch of
 * B frames [B,H,W,3], on buffers the caller owns (tests/test_tile_map_gpu.py) - the kernels every tiled film_interpolate /
 * film_interpolate_sequence / film_stream_push moves its pixels with, reached through the same dispatch.  The geometry is what those calls
 * resolve for (H, W, align, block_h, block_w) and the handle's current "block_overlap_*" (film_tiling_json describes it), with the same refusals.
 * frames_dev: the frame batch, a DEVICE pointer: float32 with FILM_PIX_F32; with FILM_PIX_U8 (cut only) bytes that the cut dequantises as
 * u8 / 255.0f - the pointer must then be 4-byte aligned and its allocation a whole number of 32-bit words, as the stream's own frame buffer
 * is: the kernel reads the aligned words that hold a row's bytes.  tiles_dev: DEVICE float32 [ntiles][padded_h][padded_w][3]; tile n of the
 * batch is at index n - tile0.  A cut writes all of tiles_dev[0, ntiles) (+0.0 in the padding) and nothing else.  A join writes only frame
 * pixels that a tile of the range covers: with overlap 0 the patches of the range; with an overlap the cross-fade - a range that starts
 * behind a pixel's first covering tile goes on from the value in the frame, so the ranges of a frame are applied in tile order.
 * Asynchronous on `stream` (a hipStream_t; NULL: the default stream).  Needs a device but no weights and no film_finalize; builds no plan and
 * touches no workspace.  FILM_ERR_INVALID (checked first, so also on a plan-only handle): a NULL pointer, mode not 0 / 1, pix not
 * FILM_PIX_F32 / FILM_PIX_U8, FILM_PIX_U8 with a join, B, H or W < 1, the refusals of the geometry, ntiles < 1 or a range outside
 * [0, B * block_h * block_w).  Then FILM_ERR_NO_DEVICE on a plan-only handle.  Not on any forward path. */
int film_debug_tile_map(film_t* h, int mode, int pix, void* frames_dev, float* tiles_dev, int B, int H, int W, int align, int block_h,
                        int block_w, int tile0, int ntiles, void* stream);
/* film_debug_segment_copy: ONE launch of the kernel a grouped stream restores and saves its carry with ("Tile groups"), on buffers the caller
 * owns (tests/test_segment_copy_gpu.py): segs = n x {source float offset, destination float offset, count} (int64, HOST array), n = 0 .. 32;
 * dst_dev[d .. d + count) = src_dev[s .. s + count) for each, bit for bit, and nothing else is written.  Offsets and counts are arbitrary (a
 * segment may start at any float and have any length, 0 included); the segments must not overlap each other and lie inside the caller's
 * allocations.  Asynchronous on `stream` (NULL: the default stream).  Takes no handle and needs no weights.  FILM_ERR_INVALID: n outside
 * 0 .. 32, a NULL pointer with n > 0, a negative offset or count, a pointer that is not 4-byte aligned.  Not on any forward path of a
 * one-group stream. */
int film_debug_segment_copy(const int64_t* segs, int n, const float* src_dev, float* dst_dev, void* stream);
/* film_debug_yuv_cut: ONE cut of a batch of B Y'CbCr frames (frame b at sample b * S of frames_dev, S = 3 H W / 2, 2 H W or 3 H W samples of one or two bytes,
 * a 4-byte aligned DEVICE pointer into an allocation of whole 32-bit words) into float32 RGB tiles: film_debug_tile_map mode 0 with pix =
 * a Y'CbCr layout (FILM_PIX_I420 / NV12 / I422 / I444 / I010 / P010 / I210 / I410) plus colour flags - same geometry, same tile buffer, same refusals (and those of `pix` above), reached through the
 * dispatch a 4:2:0 stream's push cuts with (tests/test_yuv_gpu.py).  Not on any forward path. */
int film_debug_yuv_cut(film_t* h, int pix, void* frames_dev, float* tiles_dev, int B, int H, int W, int align, int block_h, int block_w,
                       int tile0, int ntiles, void* stream);

/* The per-image evaluation metrics of the benchmark loop on the device: the reference's losses/losses.py:72-113 (l1, l2, psnr, ssim
 * of eval/eval_cli.py:160-170), restated in frame-interpolation_amd/eval/metrics.py, whose arithmetic the kernels follow (float32
 * differences for l1 / l2, float64 differences for psnr, float64 SSIM: 11-tap Gaussian window, sigma 1.5, 'VALID', k1 0.01, k2 0.03).
 * pred, ref: float32 [B,H,W,C], C = 1 or 3.  `flags`: the FILM_METRIC_* bits of the metrics to compute, + FILM_METRIC_CLIP to clip pred to
 * [0,1] first (np.clip of the eval loop).  out: HOST array [B][4] of double = {sum |d| (f32 d), sum d*d (f32 d), psnr dB, ssim};
 * entries not asked for = NaN; psnr = +inf for identical images.  mem_kind / stream as for film_forward (with FILM_MEM_DEVICE pred
 * and ref are device pointers, out stays a host array).  Synchronises the stream it ran on before returning.  Deterministic: image k
 * gives the same bits on every run, alone or in a batch, from host or device memory.  Works on any handle with a device: no weights
 * and no film_finalize needed; the handle owns the scratch.  FILM_ERR_INVALID: B <= 0, H or W <= 0, C not 1 / 3, a NULL pointer,
 * max_val <= 0, unknown flag bits, H or W < 11 with FILM_METRIC_SSIM (metrics.ssim's refusal). */
#define FILM_METRIC_L1 1
#define FILM_METRIC_L2 2
#define FILM_METRIC_PSNR 4
#define FILM_METRIC_SSIM 8
#define FILM_METRIC_CLIP 16 /* clip pred to [0,1] first */
int film_image_metrics(film_t* h, const float* pred, const float* ref, int B, int H, int W, int C, int flags, double max_val,
                       double* out, int mem_kind, void* stream);

/* write_image's quantisation on the device (replaces the host loop of the reference's eval/util.py:44-59 write_image,
 * lines 51-52): dst[i] = uint8(clip(src[i] * 255, 0, 255) + 0.5), the same float32 operations in the same order = the same bytes.
 * src (float32) and dst (uint8) are DEVICE pointers to n values; asynchronous on `stream` (NULL: the default stream) of the
 * current device.  The frames of a recursion then cross PCIe as 1 byte per value instead of 4.  Returns FILM_OK or a negative error. */
int film_to_uint8(const float* src, unsigned char* dst, int64_t n, void* stream);

/* "Out" of the 4:2:0 arithmetic above on the device: src float32 [H][W][3] -> dst, one frame of H * W * 3 / 2 samples in the layout and
 * colour setting `pix` names (FILM_PIX_I420 / FILM_PIX_NV12: bytes; FILM_PIX_I010 / FILM_PIX_P010: 16-bit words; plus flags).  DEVICE pointers, any
 * alignment of dst for the 8-bit layouts, 2-byte alignment for the 10-bit ones (else FILM_ERR_INVALID; whole 32-bit words are
 * stored where it allows); asynchronous on `stream` (NULL: the default stream) of the current device, like film_to_uint8.  What a 4:2:0
 * stream's push quantises its result with; results of film_interpolate / film_interpolate_sequence leave as 4:2:0 through it too.
 * FILM_ERR_INVALID: a NULL pointer, H or W < 1 or odd, pix no 4:2:0 pixel type (FILM_YUV_BT2020 is accepted; the 4:2:2 / 4:4:4 layouts are film_to_yuv's). */
int film_to_yuv420(const float* src, void* dst, int H, int W, int pix, void* stream);
/* film_to_yuv420's contract for EVERY Y'CbCr layout: "Out" of the layout's arithmetic, one frame of S samples (4:2:0: 3 H W / 2, H and W even; 4:2:2:
 * 2 H W, W even; 4:4:4: 3 H W, any size), bytes or 16-bit words (dst then 2-byte aligned).  What a Y'CbCr stream's push quantises its result with.
 * FILM_ERR_INVALID: a NULL pointer, H or W < 1, a size the layout refuses, an odd 10-bit dst, pix no Y'CbCr pixel type. */
int film_to_yuv(const float* src, void* dst, int H, int W, int pix, void* stream);

/* The variable-restore half of `tf.compat.v2.saved_model.load(model_path)` (reference eval/interpolator.py:148): reads the
 * checkpoint of a Keras SavedModel - `<path>/variables/variables.index` + `.data-0000N-of-0000M`, written by model.save()
 * (training/train_lib.py:280, training/build_saved_model_cli.py:65-73) - without TensorFlow and without Python, places every
 * film_net tensor (film_set_weight) and finalizes the handle (film_finalize).  `path`: the SavedModel directory, or a bundle
 * prefix (".../variables").  Tensors are found by their Keras object-graph attribute paths (extract_sublevels/convs/i,
 * _predictors/p/_convs/j, convs/i/j, output_conv - the names in feature_extractor.py:118-123,160, pyramid_flow_estimator.py:
 * 74-83,111-123, fusion.py:64-101), independent of the layer_with_weights-N numbering; a tensor not found that way is taken
 * by shape ONLY if its shape is unique among the unplaced tensors and the unused variables - anything ambiguous is an error,
 * never a guess.  verify_crc != 0 checks the masked crc32c of every index block and tensor.  report (may be NULL) receives
 * one line per tensor, "<name>\t<path|shape>\t<checkpoint key>\n" (size query: capacity 0, *needed = bytes incl. NUL).
 * Errors: FILM_ERR_NOTFOUND (no bundle at `path`, a tensor missing), FILM_ERR_INVALID (corrupt / unsupported file, crc). */
int film_load_bundle(film_t* h, const char* path, int verify_crc, char* report, int64_t report_capacity, int64_t* report_needed);

/* CRC-32C (Castagnoli) continued from `crc` (0 to start) over n bytes.  Host helper of the TF-free SavedModel
 * variables reader (frame-interpolation_amd/film_hip/tf_bundle.py), which checks the masked crc32c TensorFlow
 * stores per tensor and per index block; part of replacing tf.saved_model.load (eval/interpolator.py:148). */
uint32_t film_crc32c(uint32_t crc, const void* data, int64_t n);

/* Library build info: "gfx950;film_hip r<round>;src=<12 hex digits of the sha1 over csrc/ and this header>[+extra]" ("+extra": built
 * with FILM_EXTRA_FAMILIES=1, i.e. with the opt-in kernel families).  Tune caches, bench lines and PMC summaries carry it. */
const char* film_version(void);

#ifdef __cplusplus
}
#endif
#endif /* FILM_HIP_H_ */
