/*
 * fav.h -- C ABI of libfav: the MI355X-native (gfx950, hand-written HIP) implementation of the
 * per-frame hot path of manuelruder/fast-artistic-videos:
 *
 *   frames + backward .flo (+ forward .flo | .pgm certainty) + .t7 weights
 *     -> warp previous stylised frame -> occlusion/consistency mask -> 7-channel assembly
 *     -> conv-InstanceNorm-ReLU residual transformer network -> deprocess -> stylised frame
 *
 * Every entry point cites the reference interface it replaces (paths relative to the reference
 * tree).  Conventions:
 *   - plain C, no exceptions / longjmp across the boundary; return 0 (FAV_OK) or a negative
 *     fav_status; fav_last_error() gives a thread-local message.
 *   - all data pointers are DEVICE pointers unless the parameter name ends in `_host`;
 *     the caller owns every buffer it passes.
 *   - `stream` is a hipStream_t passed as void*; kernels are enqueued on it and the call returns
 *     without synchronising (NULL = the default stream).
 *   - concurrency: a fav_net owns one activation arena and one stream-K workspace, so it executes ONE forward at a time --
 *     everything that shares a net (its fav_streams, a fav_vr) must be enqueued on the same HIP stream or be ordered by the
 *     caller.  The persistent / stream-K convolution kernels size their grids to the whole device (minus the CUs reserved for
 *     the library's own look-ahead queues) and hand partial tiles between co-resident blocks: two forwards must therefore not
 *     run CONCURRENTLY on one device.  Inside one process the library sees to that itself: when a forward is enqueued on another
 *     HIP stream than the previous forward on that device, the host first waits for that previous stream to drain (the ONE case in
 *     which an entry point synchronises), so several nets / streams are SERIALISED, never wrong.  Before a HIP stream that carried
 *     forwards is destroyed, call fav_stream_destroy on the fav_streams that ran on it or fav_net_forget_stream (either drains it
 *     and drops the library's note of the handle).  Across processes it cannot: one process per GPU (as
 *     bench.py and the launcher do), or fav_net_set_shared_device.  Handles are not locked: do not call into the same handle
 *     from two host threads at once.
 *   - there is NO CPU fallback: without a usable HIP device every compute entry point fails with
 *     FAV_ENODEVICE.
 */
#ifndef FAV_H
#define FAV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* fav_hipstream_t;

enum fav_status {
    FAV_OK = 0,
    FAV_EINVAL = -1,       /* bad argument (shape, null pointer, ...) */
    FAV_EIO = -2,          /* file could not be opened / read / written */
    FAV_EFORMAT = -3,      /* malformed .t7 / .flo / pnm */
    FAV_EUNSUPPORTED = -4, /* valid input, but outside what the kernels cover (e.g. asymmetric reflection padding) */
    FAV_EHIP = -5,         /* HIP runtime error */
    FAV_ENODEVICE = -6     /* no HIP device: the product path has no CPU fallback */
};

/* border policy of the warp: the reference has two (fast_artistic_video/utils.lua:141-149) */
enum fav_border {
    FAV_BORDER_STN = 0, /* GPU path: stnbdhw/BilinearSamplerBDHW.cu:48-109, each tap zeroed individually */
    FAV_BORDER_CPU = 1  /* CPU path: image.warp(img, flow, 'bilinear', true, 'pad', 0) */
};

const char* fav_last_error(void);
int fav_version(void);
/* number of HIP devices, or FAV_ENODEVICE */
int fav_device_count(void);

/* ---- A2: optical-flow warp -------------------------------------------------------------------
 * Replaces nn.BilinearSamplerBDHW():forward({img, flow}) (stnbdhw/BilinearSamplerBDHW.lua:54-82,
 * native cunn_BilinearSamplerBDHW_updateOutput, stnbdhw/BilinearSamplerBDHW.cu:111-152) and the
 * CPU branch of utils.warp_image (fast_artistic_video/utils.lua:147).
 * img [B][C][H][W], flow [B][2][Ho][Wo] with flow[:,0]=dy, flow[:,1]=dx (pixel offsets),
 * out [B][C][Ho][Wo]; all contiguous fp32. */
int fav_warp_bdhw_f32(const float* img, const float* flow, float* out,
                      int B, int C, int H, int W, int Ho, int Wo,
                      int border_mode, fav_hipstream_t stream);

/* ---- A3/A4: forward-backward consistency mask ------------------------------------------------
 * Replaces the process `consistencyChecker flow1.flo flow2.flo out.pgm [image.ppm]`
 * (consistencyChecker/consistencyChecker.cpp:136-171; checkConsistency :80-134, computeCorners
 * :39-78).  flow1_flo / flow2_flo are the .flo payloads: [H][W][2] interleaved (u,v) fp32.
 * rgb_hwc is the P6 payload [H][W][3] u8, or NULL for the 3-argument mode.  out is the PGM
 * payload: [H][W] u8 in {0,255}, bit-exact with the reference binary.
 * workspace: fav_consistency_workspace_bytes(W,H,with_structure) bytes of device memory (may be
 * NULL when that returns 0). */
size_t fav_consistency_workspace_bytes(int W, int H, int with_structure);
int fav_consistency_u8(const float* flow1_flo, const float* flow2_flo, const uint8_t* rgb_hwc,
                       uint8_t* out, int W, int H, void* workspace, size_t workspace_bytes,
                       fav_hipstream_t stream);

/* test / tool entry: the structure map of the 4-argument mode itself -- computeCorners(image, 3.0f) + CMatrix::normalize(0, 1)
 * (consistencyChecker.cpp:39-78,158-159) into structure_out [H][W] fp32 and its CMatrix::avg() into avg_out [1], both device memory,
 * bit-exact with the reference binary.  rgb_hwc, workspace (fav_consistency_workspace_bytes(W, H, 1) bytes): as for fav_consistency_u8.
 * pack_cus == 0: the wide launch form, as fav_consistency_u8 runs it.  pack_cus 1..4: the packed form of the look-ahead path
 * (fav_stream_prefetch_mask) with that many working blocks; q0 (0..7) is written, in stream order, into the device word the packed
 * kernels read as "the XCD the network's queue deals block 0 to".  Called stand-alone the eight blocks of each launch land one per
 * XCD, so every q0 is a valid placement and gives the same bits.  *form_ran (host) receives the form that was launched: a device that
 * does not present eight XCDs runs the wide form whatever pack_cus says.  Enqueues on `stream` and returns; the first packed call on
 * a device synchronises `stream` once (the XCD probe).  FAV_EINVAL (nothing written) for a null pointer, W < 2, H < 2, a short
 * workspace, pack_cus or q0 out of range. */
enum fav_structure_form { FAV_STRUCTURE_WIDE = 0, FAV_STRUCTURE_PACKED = 1 };
int fav_structure_f32(const uint8_t* rgb_hwc, int W, int H, void* workspace, size_t workspace_bytes,
                      float* structure_out, float* avg_out, int pack_cus, int q0, int* form_ran,
                      fav_hipstream_t stream);

/* ---- A5: certainty erosion -------------------------------------------------------------------
 * Replaces utils.min_filter(cert, r) (fast_artistic_video/utils.lua:161-169):
 * 1 - maxpool_{r x r, stride 1, pad r/2}(1 - cert), window truncated at the borders. cert [H][W]. */
int fav_min_filter_f32(const float* cert, float* out, int H, int W, int r, fav_hipstream_t stream);

/* ---- bicubic resampling ------------------------------------------------------------------------
 * image.scale(src, Wd, Hd, 'bicubic') on a float tensor [Torch7 `image`, recalled: the package is not vendored], the resampling
 * behind -scale_factor (fast_artistic_video_core.lua:128,151).  Separable, the width first into an fp32 intermediate; along an axis
 * scale = (float)(src_len-1)/(float)(dst_len-1), sample di < dst_len-1 is the Catmull-Rom cubic through s[i-1..i+2] at
 * x = di*scale - i (i = floor), with the missing neighbour at either end extrapolated linearly (2*p1 - p2, 2*p2 - p1); the last sample
 * is s[src_len-1]; equal lengths copy; a one-sample source is repeated.  No clamping, no antialiasing, any factor.
 * src [C][Hs][Ws], dst [C][Hd][Wd], contiguous fp32, device pointers. */
int fav_scale_bicubic_f32(const float* src, float* dst, int C, int Hs, int Ws, int Hd, int Wd, fav_hipstream_t stream);

/* ---- dense optical flow ------------------------------------------------------------------------
 * Stands in for `run-deepflow.sh <img1> <img2> <out.flo>` (makeOptFlow_deepflow.sh:46-49: two closed CPU binaries) with a variational
 * estimator WITHOUT descriptor matching: Horn-Schunck with warping, coarse to fine, Jacobi sweeps, all in fp32 (the algorithm is stated
 * in DESIGN.md, "fav_flow", and restated in numpy by tests/util/flow_model.py).  It recovers the small and medium motions of consecutive
 * video frames; motions much larger than the coarsest level represents (about 2^levels pixels) are not recovered, and its quality
 * against DeepFlow is unmeasured.
 * The flow "from A to B" is w with B(p + w(p)) ~ A(p): flow_out is the .flo payload [H][W][2] (u, v), what fav_stream_next_frame_flow
 * takes.  a_rgb_hwc / b_rgb_hwc: P6 payloads [H][W][3] u8.  Every field of fav_flow_opts may be 0 = default (levels: while the smaller
 * side is still >= 16, at most 6; warps 3; iters 30; alpha 15 grey levels; sweeps_per_launch 6 -- the number of Jacobi sweeps a launch
 * runs on a tile in LDS, 1..16: the result is bit-identical for every value); opts_host may be NULL.
 * workspace: fav_flow_workspace_bytes(W, H, opts) bytes of device memory, 16-byte aligned, owned by the caller, private to the call until
 * the stream has passed it (0 with a message: bad size or options).  The call allocates nothing and does not synchronise.
 * W, H >= 16; anything else, or an option out of range, is FAV_EINVAL.
 * smooth_eps = eps > 0 makes the smoothness term EDGE-PRESERVING ("Edge-preserving smoothness"; restated by
 * tests/util/flow_robust_model.py): every warp weights the four neighbours of a pixel with the lagged diffusivity
 * g = 1 / sqrt(|grad u0|^2 + |grad v0|^2 + eps^2) of its starting flow, so the flow is no longer smeared across motion boundaries; with
 * g = 1 it is the quadratic term, and alpha keeps its meaning.  alpha 0 then means 5; 0.3 is the measured choice for eps.  0 = off: the
 * estimator, its launches and its workspace are what they were.  Negative, non-finite, or outside 1e-6 .. 1e6: FAV_EINVAL.  The workspace
 * grows by one weight image of 16 bytes per pixel and flow.  fav_flow_rgb8, fav_flow_pairs_rgb8 and fav_stream_next_frame_estimate honour
 * the field.
 * THE STRUCT GREW by this trailing field (24 bytes, was 20): a caller compiled against the earlier header passes a shorter struct and must
 * be rebuilt; every in-tree user (bin/, python/fav_amd) is. */
typedef struct fav_flow_opts { int levels; int warps; int iters; float alpha; int sweeps_per_launch; float smooth_eps; } fav_flow_opts;
size_t fav_flow_workspace_bytes(int W, int H, const fav_flow_opts* opts_host);
int fav_flow_rgb8(const uint8_t* a_rgb_hwc, const uint8_t* b_rgb_hwc, int W, int H, const fav_flow_opts* opts_host,
                  float* flow_out, void* workspace, size_t workspace_bytes, fav_hipstream_t stream);
/* Both flows of n_pairs (1..FAV_FLOW_MAX_PAIRS) frame pairs of one size in ONE sequence of launches (every launch works on all 2 n_pairs
 * flows; the grey pyramid of each of the 2 n_pairs images is built once and serves both directions): what the six cube faces of a
 * 360-degree frame need.  The four arrays are HOST arrays of n_pairs device pointers; an image may appear in more than one slot.
 *   backward_flo[k]: the flow with A = cur[k], B = prev[k];  forward_flo[k]: the flow with A = prev[k], B = cur[k]
 * (the two flows of fav_stream_next_frame_estimate), each bit-identical to what fav_flow_rgb8 writes for the same (A, B, options), for
 * every n_pairs.  Workspace and contract as fav_flow_rgb8 with fav_flow_pairs_workspace_bytes; the 2 n_pairs outputs are 8-byte aligned
 * and distinct.  The call may run on several streams at once (with a workspace each). */
#define FAV_FLOW_MAX_PAIRS 8
size_t fav_flow_pairs_workspace_bytes(int W, int H, int n_pairs, const fav_flow_opts* opts_host);
int fav_flow_pairs_rgb8(const uint8_t* const* prev_rgb_hwc, const uint8_t* const* cur_rgb_hwc, int n_pairs, int W, int H,
                        const fav_flow_opts* opts_host, float* const* backward_flo, float* const* forward_flo,
                        void* workspace, size_t workspace_bytes, fav_hipstream_t stream);
/* The extended options: fav_flow_opts (which keeps its 24 bytes) plus the DATA TERM.  FAV_FLOW_DATA_BRIGHTNESS (0) compares grey levels, as
 * ever; FAV_FLOW_DATA_GRADIENT (1) compares the image gradients INSTEAD (gradient constancy, Brox et al. 2004; DESIGN.md, "Gradient-
 * constancy data term"; restated by tests/util/flow_grad_model.py), so a change of exposure between the two frames -- gain, offset, a slow
 * ramp -- is not read as motion; in constant light it costs a few hundredths of a pixel.  Any other value is FAV_EINVAL.  alpha 0 then
 * means 8, with smooth_eps > 0 as well.  The workspace holds 20 instead of 16 bytes of coefficients per pixel and flow.  Every entry
 * without _ex is its _ex twin with data_term 0: the same bits, launches and workspace. */
#define FAV_FLOW_DATA_BRIGHTNESS 0
#define FAV_FLOW_DATA_GRADIENT 1
typedef struct fav_flow_opts_ex { fav_flow_opts base; int data_term; } fav_flow_opts_ex;
size_t fav_flow_workspace_bytes_ex(int W, int H, const fav_flow_opts_ex* opts_host);
int fav_flow_rgb8_ex(const uint8_t* a_rgb_hwc, const uint8_t* b_rgb_hwc, int W, int H, const fav_flow_opts_ex* opts_host,
                     float* flow_out, void* workspace, size_t workspace_bytes, fav_hipstream_t stream);
size_t fav_flow_pairs_workspace_bytes_ex(int W, int H, int n_pairs, const fav_flow_opts_ex* opts_host);
int fav_flow_pairs_rgb8_ex(const uint8_t* const* prev_rgb_hwc, const uint8_t* const* cur_rgb_hwc, int n_pairs, int W, int H,
                           const fav_flow_opts_ex* opts_host, float* const* backward_flo, float* const* forward_flo,
                           void* workspace, size_t workspace_bytes, fav_hipstream_t stream);
/* The options with the MATCHING PRIOR ("Matching prior"; restated by tests/util/flow_match_model.py): fav_flow_opts_ex (which
 * keeps its 28 bytes) plus match_beta and match_radius.  match_beta 0 = off: the _ex entry's launches, workspace and bits.  With
 * match_beta > 0 (up to 1e6; negative = the default, 225) both frames are block-matched at pyramid level 1 -- integer sums of absolute
 * differences over 7 x 7 windows of the rounded grey, displacements in [-match_radius, match_radius]^2 (1..32; 0 = the default, 16, i.e.
 * +-32 px at full size), forward-backward checked -- and wherever a warp's starting flow is further than a threshold from a confirmed
 * match the data term gains a quadratic pull of weight match_beta towards it: objects that move further than their own size, which the
 * pyramid alone loses, are recovered, at the price of about 0.1 px where nothing moves far (the matches are integers at half
 * resolution), so it is off by default.  It combines with smooth_eps and data_term.  A pyramid of a single level has no level 1:
 * FAV_EINVAL.  The workspace grows by the match fields, the prior's pyramid and, with the brightness term, 4 bytes of coefficients per
 * pixel and flow.  Every _ex entry is its _ex2 twin with match_beta 0. */
typedef struct fav_flow_opts_ex2 { fav_flow_opts_ex ex; float match_beta; int match_radius; } fav_flow_opts_ex2;
size_t fav_flow_workspace_bytes_ex2(int W, int H, const fav_flow_opts_ex2* opts_host);
int fav_flow_rgb8_ex2(const uint8_t* a_rgb_hwc, const uint8_t* b_rgb_hwc, int W, int H, const fav_flow_opts_ex2* opts_host,
                      float* flow_out, void* workspace, size_t workspace_bytes, fav_hipstream_t stream);
size_t fav_flow_pairs_workspace_bytes_ex2(int W, int H, int n_pairs, const fav_flow_opts_ex2* opts_host);
int fav_flow_pairs_rgb8_ex2(const uint8_t* const* prev_rgb_hwc, const uint8_t* const* cur_rgb_hwc, int n_pairs, int W, int H,
                            const fav_flow_opts_ex2* opts_host, float* const* backward_flo, float* const* forward_flo,
                            void* workspace, size_t workspace_bytes, fav_hipstream_t stream);
/* The options with the MEDIAN FILTER ("Median filtering"; restated by tests/util/flow_median_model.py): fav_flow_opts_ex2 (which
 * keeps its 36 bytes) plus median.  median 0 = off: the _ex2 entry's launches and bits.  median 3 or 5 is the side of a window: after the
 * sweeps of every warp at every level -- the last warp of level 0 included -- u and v are replaced, each on its own, by the median of their
 * 3 x 3 (the 5th smallest of 9) or 5 x 5 (the 13th smallest of 25) neighbourhood, neighbour indices clamped to the image (Sun, Roth and
 * Black, "Secrets of optical flow estimation", 2010).  The filtered flow is what the next warp linearises around, what the next finer
 * level upsamples and, at level 0, what the caller receives.  A median removes the isolated outliers of a warp step, which the linear
 * smoothness term only spreads, and keeps motion boundaries; it is pure selection, so the stage equals a sort value for value.  What it
 * gains and costs is measured in DESIGN.md; it is off by default.  It combines with smooth_eps, data_term and match_beta.  Any other
 * value is FAV_EINVAL (workspace query: 0) with a message that names it.  The filter alternates between the two flow buffers a level
 * already has: the workspace is the _ex2 entry's, byte for byte.  Every _ex2 entry is its _ex3 twin with median 0. */
typedef struct fav_flow_opts_ex3 { fav_flow_opts_ex2 ex2; int median; } fav_flow_opts_ex3;
size_t fav_flow_workspace_bytes_ex3(int W, int H, const fav_flow_opts_ex3* opts_host);
int fav_flow_rgb8_ex3(const uint8_t* a_rgb_hwc, const uint8_t* b_rgb_hwc, int W, int H, const fav_flow_opts_ex3* opts_host,
                      float* flow_out, void* workspace, size_t workspace_bytes, fav_hipstream_t stream);
size_t fav_flow_pairs_workspace_bytes_ex3(int W, int H, int n_pairs, const fav_flow_opts_ex3* opts_host);
int fav_flow_pairs_rgb8_ex3(const uint8_t* const* prev_rgb_hwc, const uint8_t* const* cur_rgb_hwc, int n_pairs, int W, int H,
                            const fav_flow_opts_ex3* opts_host, float* const* backward_flo, float* const* forward_flo,
                            void* workspace, size_t workspace_bytes, fav_hipstream_t stream);
/* the filter on its own: flow_in -> flow_out, both [H][W][2], 8-byte aligned, size 3 or 5.  Not in place: buffers that overlap, or another
 * size, are FAV_EINVAL with a message. */
int fav_flow_median_f32(const float* flow_in, float* flow_out, int W, int H, int size, fav_hipstream_t stream);
/* the prior's stages on their own.  fav_flow_match_f32: two grey planes [H][W] -> the match fields of both directions, d_ab / d_ba
 * [H][W][2] int16 (dx, dy), 4-byte aligned (radius 1..32).  fav_flow_match_check: the forward-backward test of d_ab against d_ba ->
 * prior, THREE PLANES [3][H][W] fp32 (d_ab.x, d_ab.y, m) with m 0 | 1.  fav_flow_coefficients_prior_f32: one warp's coefficients with
 * a prior -- coef is the five planes of fav_flow_coefficients_grad_f32 with either data_term; prior [3][Hp][Wp] is the level's own
 * (Wp = W, Hp = H) or the next coarser level's (Wp = ceil(W/2), Hp = ceil(H/2): level 0 reading level 1); beta in (0, 1e6], tau >= 0 the
 * gate (the estimator: 1, at level 0: 2); weights NULL or as in the _grad_ entry. */
int fav_flow_match_f32(const float* a_grey, const float* b_grey, int W, int H, int radius, int16_t* d_ab, int16_t* d_ba, fav_hipstream_t stream);
int fav_flow_match_check(const int16_t* d_ab, const int16_t* d_ba, int W, int H, float* prior, fav_hipstream_t stream);
int fav_flow_coefficients_prior_f32(const float* a_grey, const float* b_grey, const float* flow0, float alpha, float smooth_eps, int data_term,
                                    const float* prior, int Wp, int Hp, float beta, float tau, float* coef, float* weights, int W, int H,
                                    fav_hipstream_t stream);
/* the estimator's stages on their own (operator-level entries, as fav_scale_bicubic_f32 is one): the grey image [H][W]; one pyramid step
 * to ceil(W/2) x ceil(H/2); the x2 flow upsampling between two level sizes; the coefficients (a, b, c, r) of one warp around flow0,
 * [H][W][4], 16-byte aligned; `iters` Jacobi sweeps from flow0 into flow_out (scratch: a second flow buffer [H][W][2]; flow0 is not
 * written and must be neither of the two).
 * The _robust_ pair is one warp of the edge-preserving smoothness (smooth_eps > 0): the coefficients (r with the weights' sum in it) plus
 * the four normalised edge weights (n_left, n_right, n_up, n_down), [H][W][4], 16-byte aligned, and the sweeps that use them. */
int fav_flow_grey_f32(const uint8_t* rgb_hwc, float* grey, int W, int H, fav_hipstream_t stream);
int fav_flow_down_f32(const float* src, float* dst, int W, int H, fav_hipstream_t stream);
int fav_flow_up_f32(const float* coarse_flow, int Wc, int Hc, float* fine_flow, int W, int H, fav_hipstream_t stream);
int fav_flow_coefficients_f32(const float* a_grey, const float* b_grey, const float* flow0, float alpha, float* coef, int W, int H,
                              fav_hipstream_t stream);
int fav_flow_sweeps_f32(const float* flow0, const float* coef, int iters, int sweeps_per_launch, float* flow_out, float* scratch,
                        int W, int H, fav_hipstream_t stream);
int fav_flow_coefficients_robust_f32(const float* a_grey, const float* b_grey, const float* flow0, float alpha, float smooth_eps, float* coef,
                                     float* weights, int W, int H, fav_hipstream_t stream);
int fav_flow_sweeps_robust_f32(const float* flow0, const float* coef, const float* weights, int iters, int sweeps_per_launch, float* flow_out,
                               float* scratch, int W, int H, fav_hipstream_t stream);
/* The _grad_ pair is one warp of the gradient-constancy data term: coef is FIVE PLANES [5][H][W] (q11, q12, q22, e1, e2), 4-byte aligned --
 * the per-pixel 2 x 2 system already solved, so that a sweep is u = (q11 u_bar + q12 v_bar) + e1, v = (q12 u_bar + q22 v_bar) + e2.
 * weights NULL: the quadratic smoothness term and the plain mean (smooth_eps is not read); otherwise the edge-preserving smoothness, with
 * the weights written by the coefficients and read by the sweeps as in the _robust_ pair. */
int fav_flow_coefficients_grad_f32(const float* a_grey, const float* b_grey, const float* flow0, float alpha, float smooth_eps, float* coef,
                                   float* weights, int W, int H, fav_hipstream_t stream);
int fav_flow_sweeps_grad_f32(const float* flow0, const float* coef, const float* weights, int iters, int sweeps_per_launch, float* flow_out,
                             float* scratch, int W, int H, fav_hipstream_t stream);

/* ---- A6/A7: VGG preprocessing + 7-channel input assembly --------------------------------------
 * Replaces run_next_image's input construction (fast_artistic_video_core.lua:161-171) and the first
 * frame's (:133-138) with fill_occlusions = vgg-mean; preprocess.lua:57-62.
 * frame_rgb [3][H][W] RGB in [0,1]; warped_rgb [3][H][W] or NULL (first frame);
 * cert [H][W] (already min-filtered) or NULL; in7 [7][H][W]. */
int fav_assemble_input_f32(const float* frame_rgb, const float* warped_rgb, const float* cert,
                           float* in7, int H, int W, fav_hipstream_t stream);

/* ---- A8: the transformer network ---------------------------------------------------------------
 * Replaces torch.load(path).model + model:forward(input) (fast_artistic_video_core.lua:38-57,172);
 * layer semantics of fast_artistic_video/models_video.lua:10-140, InstanceNormalization.lua:33-53,
 * ShaveImage.lua:9-16, train_video.lua:319-325. */
typedef struct fav_net fav_net;

/* parse a Torch7 .t7 checkpoint on the host and upload the weights to `device` */
int fav_net_create(const char* t7_path_host, int device, fav_net** out);
/* host-side: flatten a .t7 checkpoint into a self-describing blob (what rank 0 broadcasts over
 * RCCL in the multi-GPU launcher).  Call with blob_host=NULL to query the size. */
int fav_net_pack_host(const char* t7_path_host, void* blob_host, size_t capacity, size_t* bytes);
/* create a net from a packed blob (host memory) */
int fav_net_create_from_blob(const void* blob_host, size_t bytes, int device, fav_net** out);
void fav_net_destroy(fav_net* net);
/* The stream-K convolution grids hand partial tiles between co-resident blocks; a hand-off that cannot complete (another
 * context holding compute units of the device) times out inside the kernel and sets a host-visible word.  Call this AFTER the
 * work of a frame has completed (event / stream synchronised): FAV_EHIP means the frames computed since the last check are
 * wrong.  fav_stylize checks before every PNG is queued and at exit; fav_net_forward / fav_stream_* also fail on their next
 * call.  Clears the word. */
int fav_net_check(fav_net* net);
/* shared != 0: the device is NOT exclusively this network's (other processes / contexts compute on it).  The convolutions then
 * use data-parallel grids only -- one block per tile, nothing handed between blocks, no co-residency assumed -- at some cost in
 * load balance.  fav_net_check switches a network to this mode by itself after a hand-off has timed out. */
int fav_net_set_shared_device(fav_net* net, int shared);
/* `stream` (a hipStream_t that forwards of this network's device were enqueued on) is about to be destroyed by its owner: drains it
 * if it is the one the library would otherwise wait on before the next forward on another stream (concurrency note above). */
int fav_net_forget_stream(fav_net* net, fav_hipstream_t stream);
/* human-readable layer list (one line per layer) -- used to cross-check the .t7 reader */
int fav_net_describe_host(const fav_net* net, char* buf_host, size_t capacity);
/* host-only (no device needed): parse a .t7 checkpoint and write the same layer list text */
int fav_t7_describe_host(const char* t7_path_host, char* buf_host, size_t capacity);
/* number of fp32 parameters (conv weights+biases+IN gamma/beta) */
long long fav_net_param_count(const fav_net* net);
/* output size for an H x W input (equals H x W when H, W are multiples of 4) */
int fav_net_output_size(const fav_net* net, int H, int W, int* Ho, int* Wo);
/* in7 [1][7][H][W] -> out3 [1][3][Ho][Wo] (150*tanh(...), BGR mean-subtracted space), fp32 NCHW.
 * Internal buffers are (re)sized on first use for a given H x W (allocation happens outside the
 * stream order only then). */
int fav_net_forward(fav_net* net, const float* in7, float* out3, int H, int W, fav_hipstream_t stream);

/* per-convolution timing with HIP events recorded on the forward's stream (bench / roofline use).
 * enable: every later forward records one event pair per convolution launch.  read: synchronises the
 * recorded events and returns, per convolution in network order, the summed milliseconds, the number of
 * launches, the useful MACs of one launch (no padding) and an id of the kernel instance that ran it (1 = row-folded
 * last layer, 8 = first-layer kernel, 300+N = halo-resident 3x3 kernel with N output channels, 800+N = transposed-convolution
 * kernel, otherwise the N tile
 * 128/64/32 of the generic implicit-GEMM kernel); then clears the accumulators.  Arrays hold up to `capacity` entries. */
int fav_net_profile_enable(fav_net* net, int on);
int fav_net_profile_read_host(fav_net* net, int capacity, int* count, double* ms_sum, int* launches,
                              double* macs_per_launch, int* ntile);

/* operator-level entry (nn.SpatialConvolution [+ nn.InstanceNormalization [+ nn.ReLU]]), NCHW fp32;
 * weight [Cout][Cin][k][k], bias [Cout] or NULL, gamma/beta [Cout] or NULL (no IN).
 * Runs the same MFMA implicit-GEMM kernel the network uses.  Allocates temporaries: test/ops use. */
int fav_conv2d_nchw_f32(const float* in, int Cin, int H, int W,
                        const float* weight, const float* bias, int Cout, int k, int stride, int pad,
                        const float* gamma, const float* beta, float eps, int relu,
                        float* out, fav_hipstream_t stream);

/* operator-level entry (nn.SpatialFullConvolution [+ nn.InstanceNormalization [+ nn.ReLU]]), NCHW fp32, same conventions;
 * weight [Cin][Cout][k][k]; output (H - 1) * stride - 2 * pad + k + adj per axis.  k <= 9, stride <= 4, pad <= k - 1, adj < stride.
 * Stride >= 2 runs the phase-decomposed MFMA kernel the network uses for `u<n>` / `f<k>s<s>-<n>` layers, stride 1 the ordinary
 * convolution it is.  Allocates temporaries: test/ops use. */
int fav_conv_transpose2d_nchw_f32(const float* in, int Cin, int H, int W,
                                  const float* weight, const float* bias, int Cout, int k, int stride, int pad, int adj,
                                  const float* gamma, const float* beta, float eps, int relu,
                                  float* out, fav_hipstream_t stream);

/* ---- the fused per-frame pipeline (A1..A10 minus file I/O) -------------------------------------
 * Replaces one iteration of run_fast_neural_video's loop (fast_artistic_video_core.lua:194-211)
 * with the video CLI's callbacks (fast_artistic_video.lua:93-172).  Holds the recurrent state
 * last_frame_stylized (float, unclamped: fast_artistic_video.lua:169) on the device. */
/* Arithmetic of the network.  FAV_PRECISION_FP32 (default) is the parity mode: fp32 operands, exact fp32 MFMA.  The optional
 * fast mode FAV_PRECISION_BF16_OPERANDS rounds the operands of the halo-resident 3x3 convolutions (the
 * residual blocks and c3s1-64: 71 % of the FLOPs) to bf16 on their way into LDS, accumulates in fp32 and keeps every
 * activation in fp32; it is NOT bit-compatible with the reference and is gated by PSNR against the fp32 oracle in the tests. */
enum fav_precision { FAV_PRECISION_FP32 = 0, FAV_PRECISION_BF16_OPERANDS = 1 };
int fav_net_set_precision(fav_net* net, int mode);

typedef struct fav_stream fav_stream;

typedef struct fav_stream_opts {
    int border_mode;           /* enum fav_border */
    int occlusions_min_filter; /* -occlusions_min_filter (default 7): 1..15, below 1 runs as 1, above 15 is FAV_EINVAL at create */
    int invert_occlusion;      /* -invert_occlusion */
    int fix_occlusions;        /* -fix_occlusions */
    int fill_random;           /* -fill_occlusions uniform-random (1) | vgg-mean (0): core.lua:108-117.  The reference's
                                  torch.rand is unseeded; here u = counter RNG(seed, frame counter, channel, y, x), see fav_vr */
    unsigned seed;
} fav_stream_opts;

/* H x W: size of the frames (= flows = certainty maps).  The stylised frame has the NETWORK's output size Ho x Wo
 * (fav_stream_output_size): equal to H x W when both are multiples of 4, up to 3 pixels larger otherwise (two stride-2
 * convolutions, two x2 upsamplings).  As in the reference, that larger image is what is saved and kept as the recurrent state, and
 * the next frame's warp samples it on the flow's H x W grid (stnbdhw/BilinearSamplerBDHW.lua:71: the output takes the grid's size;
 * stylizeVideo_deepflow.sh:72-78 lets the user pick any w:h, e.g. 854x480).  Every out_rgb_f32 below is [3][Ho][Wo], every
 * out_rgb8_hwc [Ho][Wo][3]. */
int fav_stream_create(fav_net* net, int H, int W, const fav_stream_opts* opts_host, fav_stream** out);
int fav_stream_output_size(const fav_stream* s, int* Ho, int* Wo);
void fav_stream_destroy(fav_stream* s);
/* -model_img <file>: a separate 3-channel image model (fast_artistic_video_core.lua:59-66,146) that stylises frames
 * without a prior (fav_stream_first_frame).  NULL restores 'self' (the video model with an all-occluded prior).  The
 * image model must use the same leading reflection padding as the video model.  Not owned by the stream. */
int fav_stream_set_image_net(fav_stream* s, fav_net* image_net);
/* -scale_factor (fast_artistic_video_core.lua:127-130,150-152): frames WITHOUT a prior (fav_stream_first_frame) are resampled to
 * Hs x Ws (fav_scale_bicubic_f32's arithmetic on the byte / 255 image) before the model, the model runs at that size -- the image
 * model when one is set, its padding rule unchanged -- and the de-processed result is resampled to the stream's H x W, which is
 * what is returned, saved and kept as the recurrent state.  0, 0 restores the unscaled path.  fav_stream_next_frame_* are untouched:
 * the frame after a scaled one runs at H x W on the H x W state.
 *   - the stylised frames must have the frames' size (Ho == H, Wo == W: H and W multiples of 4 for the canonical models), because
 *     the reference scales back to W x H exactly: otherwise FAV_EUNSUPPORTED;
 *   - Hs x Ws must be a size fav_stream_create would accept (larger than the reflection padding, non-empty network output):
 *     otherwise FAV_EINVAL;
 *   - the scaled input and the scaled output are buffers of the stream, allocated by this call, not per frame;
 *   - a fav_net keeps ONE activation arena: when frames at both sizes run through the same network (the video model as its own image
 *     model without -create_inconsistent) the arena is rebuilt once, when frame 2 arrives at full size;
 *   - deviation: with model_img == 'self' the reference itself stops in torch.cat (core.lua:135 builds the fill at H x W next to an
 *     Hs x Ws image).  Here the evident intent is implemented: the prior and mask planes, and the uniform-random fill's (y, x)
 *     key, are those of the scaled grid. */
int fav_stream_set_single_image_size(fav_stream* s, int Hs, int Ws);
/* first frame / -create_inconsistent: core.lua:121-158 with model_img == 'self'.
 * frame_rgb_hwc: P6 payload [H][W][3] u8.  out_rgb_f32 [3][H][W] float RGB (deprocessed, unclamped)
 * and/or out_rgb8_hwc [H][W][3] u8 (image.save quantisation); either may be NULL. */
int fav_stream_first_frame(fav_stream* s, const uint8_t* frame_rgb_hwc,
                           float* out_rgb_f32, uint8_t* out_rgb8_hwc, fav_hipstream_t stream);
/* next frame with a precomputed certainty map (the .pgm written by consistencyChecker):
 * backward_flo [H][W][2] (u,v) payload of backward_[i]_{i-1}.flo, cert_pgm [H][W] u8. */
int fav_stream_next_frame_cert(fav_stream* s, const uint8_t* frame_rgb_hwc, const float* backward_flo,
                               const uint8_t* cert_pgm, float* out_rgb_f32, uint8_t* out_rgb8_hwc,
                               fav_hipstream_t stream);
/* next frame with the consistency check fused on the GPU: forward_flo = forward_{i-1}_[i].flo.
 * use_structure != 0 selects the 4-argument (image-structure) mode of the checker. */
int fav_stream_next_frame_flow(fav_stream* s, const uint8_t* frame_rgb_hwc, const float* backward_flo,
                               const float* forward_flo, int use_structure,
                               float* out_rgb_f32, uint8_t* out_rgb8_hwc, fav_hipstream_t stream);
/* next frame from the frames alone (fav_stylize -estimate_flow 1): the backward flow (A = this frame, B = the previous one) and the
 * forward flow (A = the previous frame, B = this one) are estimated with fav_flow_rgb8 into the caller's buffers backward_flo /
 * forward_flo ([H][W][2] each) on `stream`, then the frame runs as fav_stream_next_frame_flow with them.  workspace: as fav_flow_rgb8
 * (two single estimates, one after the other), or -- better -- fav_flow_pairs_workspace_bytes(W, H, 1, opts) bytes: both flows are then
 * estimated together as the batch of one (fav_flow_pairs_rgb8: each frame's pyramid once, half the launches; the same bits). */
int fav_stream_next_frame_estimate(fav_stream* s, const uint8_t* frame_rgb_hwc, const uint8_t* prev_frame_rgb_hwc,
                                   const fav_flow_opts* flow_opts_host, int use_structure, float* backward_flo, float* forward_flo,
                                   void* workspace, size_t workspace_bytes, float* out_rgb_f32, uint8_t* out_rgb8_hwc,
                                   fav_hipstream_t stream);
/* ... with the extended flow options (fav_flow_opts_ex: the data term); workspace sizes from the _ex queries */
int fav_stream_next_frame_estimate_ex(fav_stream* s, const uint8_t* frame_rgb_hwc, const uint8_t* prev_frame_rgb_hwc,
                                      const fav_flow_opts_ex* flow_opts_host, int use_structure, float* backward_flo, float* forward_flo,
                                      void* workspace, size_t workspace_bytes, float* out_rgb_f32, uint8_t* out_rgb8_hwc,
                                      fav_hipstream_t stream);
/* ... and with the matching prior (fav_flow_opts_ex2); workspace sizes from the _ex2 queries */
int fav_stream_next_frame_estimate_ex2(fav_stream* s, const uint8_t* frame_rgb_hwc, const uint8_t* prev_frame_rgb_hwc,
                                       const fav_flow_opts_ex2* flow_opts_host, int use_structure, float* backward_flo, float* forward_flo,
                                       void* workspace, size_t workspace_bytes, float* out_rgb_f32, uint8_t* out_rgb8_hwc,
                                       fav_hipstream_t stream);
/* ... and with the median filter between warps (fav_flow_opts_ex3); workspace sizes from the _ex3 queries (the _ex2 sizes) */
int fav_stream_next_frame_estimate_ex3(fav_stream* s, const uint8_t* frame_rgb_hwc, const uint8_t* prev_frame_rgb_hwc,
                                       const fav_flow_opts_ex3* flow_opts_host, int use_structure, float* backward_flo, float* forward_flo,
                                       void* workspace, size_t workspace_bytes, float* out_rgb_f32, uint8_t* out_rgb8_hwc,
                                       fav_hipstream_t stream);
/* optional look-ahead: start computing the consistency mask of a FUTURE frame on an internal side stream (the mask
 * depends only on that frame and its two flows, not on the recurrent state), so the order-preserving 4-argument
 * structure pass overlaps the network of the current frame.  The inputs must already be complete on `stream`.  The next
 * fav_stream_next_frame_flow call with the same three pointers and mode consumes the prefetched mask.
 * A look-ahead stays pending -- across fav_stream_first_frame, fav_stream_set_state and frames that do not match it, whose results it
 * does not touch -- until it is consumed, until the fourth look-ahead after it takes its slot (four slots, dealt in turn), or until
 * fav_stream_set_host_ordered drops it; the three buffers must stay unchanged for as long. */
int fav_stream_prefetch_mask(fav_stream* s, const uint8_t* frame_rgb_hwc, const float* backward_flo,
                             const float* forward_flo, int use_structure, fav_hipstream_t stream);
/* Host-ordered look-ahead (on != 0): fav_stream_prefetch_mask then records nothing on `stream` and nothing waits on it -- the CALLER
 * guarantees that the three input buffers are complete when it calls (it has seen their upload finish) -- and the matching
 * fav_stream_next_frame_flow waits for the look-ahead on the HOST (a sequence number the mask pipeline's last kernel stores into
 * host-mapped memory; polled with short sleeps, normally already there) instead of making the compute queue wait on an event.
 * Why: on this runtime every event record behind long-running kernels and every dependency between queues keeps a runtime thread
 * spinning until it resolves -- one core per process ("quiet synchronisation").  The look-ahead's OUTPUT buffers are the
 * library's business in both modes: host-ordered, a look-ahead that would rewrite a mask / certainty buffer which frames still in the
 * caller's queue read waits on the host until those frames are through (a retire sequence number stored by a one-thread kernel in the
 * caller's queue; with up to two frames of look-ahead that is never a wait), so a caller may run any number of frames ahead.
 * Every call, in either direction, drops all pending look-aheads (the frames they were for compute their masks inline) and must be made
 * with the caller's queue drained: the retire bookkeeping starts anew, and knows nothing of frames enqueued in the other mode.
 * Default: off (event-ordered, fully asynchronous). */
int fav_stream_set_host_ordered(fav_stream* s, int on);
/* read / overwrite the recurrent state ([3][Ho][Wo] float RGB) -- for -continue_with */
int fav_stream_get_state(fav_stream* s, float* state_rgb_f32, fav_hipstream_t stream);
int fav_stream_set_state(fav_stream* s, const float* state_rgb_f32, fav_hipstream_t stream);
/* test view: the 7-channel network input of the LAST frame as run_next_image assembles it (fast_artistic_video_core.lua:161-171:
 * content | masked warped prior + fill | certainty), [7][H][W] fp32, copied out of the fused kernel's padded buffer (FAV_EINVAL
 * right after a frame that ran at the scaled single-image size) */
int fav_stream_get_input_f32(const fav_stream* s, float* in7, fav_hipstream_t stream);
/* test view: the same frame's input as the network reads it, with the leading reflection padding p the input assembly writes
 * (0 when the model starts without a symmetric reflection padding): [H + 2p][W + 2p][8] fp32, channel 7 zero -- a device-to-device
 * copy of the stream's buffer.  Same preconditions and errors as fav_stream_get_input_f32 */
int fav_stream_get_padded_input_f32(const fav_stream* s, float* out, fav_hipstream_t stream);
/* device pointer of the last certainty mask used (u8 [H][W], before the min filter) -- tests.  fav_stream_first_frame uses none and
 * leaves the buffer as it was: its content is defined after a fav_stream_next_frame_* call only */
const uint8_t* fav_stream_last_mask(const fav_stream* s);


/* fp32 sum in index order with the rounding of every partial sum: bit-identical to `float s = 0; for (i) s += x[i];`, the
 * arithmetic of CMatrix::avg (consistencyChecker/CMatrix.h:1245-1251) that the 4-argument checker depends on.  Evaluated in
 * parallel (exact parity-transducer scan; kernels_consistency.hip).  x, sum_out: device pointers. */
int fav_sequential_sum_f32(const float* x, size_t n, float* sum_out, fav_hipstream_t stream);

/* ---- temporal-consistency metric -------------------------------------------------
 * The third number of func_eval (fast_artistic_video.lua:128-151, -evaluate without the VGG terms):
 * MSE(warp(prev_stylised, flow) * cert, cur_stylised * cert) over 3*H*W elements (nn.MSECriterion).  prev / cur: [3][H][W]
 * float RGB (what fav_stream_get_state returns), backward_flo: .flo payload, cert_pgm: u8 [H][W].  Synchronises `stream`;
 * the value is written to host memory. */
int fav_temporal_loss_host(const float* prev_rgb, const float* cur_rgb, const float* backward_flo, const uint8_t* cert_pgm,
                           int H, int W, int border_mode, double* loss_host, fav_hipstream_t stream);

/* ---- 360-degree cube-map orchestration --------------------------------------------
 * Replaces the callbacks fast_artistic_video_vr.lua passes to run_fast_neural_video (fast_artistic_video_core.lua:189-229):
 * func_load_cert (:204-237), func_make_last_frame_warped (:239-302), func_is_single_image (:304-310), func_save_image /
 * blend_other_sides (:454-559), with the static maps of fast_artistic_video/vr_helper.lua:3-184.  Faces are hplus x wplus
 * (face + overlap); face index i is 1-based and frame-major, mode = (i-1) % 6 walks the processing order of file ids
 * {6,1,2,5,3,4} (:103); the caller maps ids to files.  `-fill_occlusions uniform-random` is an unseeded torch.rand in the
 * reference (core.lua:108-117); here it is a documented counter RNG keyed by (seed, i, channel, y, x). */
typedef struct fav_vr fav_vr;
typedef struct fav_vr_opts {
    int overlap_w, overlap_h;        /* -overlap_pixel_w / _h (fast_artistic_video_vr.lua:42-43); even, > 10 */
    int occlusions_min_filter;       /* :36; 1..15, below 1 runs as 1, above 15 is FAV_EINVAL at create */
    int median_filter;               /* :50; 0, 3 or 5 */
    int fill_random;                 /* -fill_occlusions uniform-random (1) | vgg-mean (0) */
    unsigned seed;                   /* of the documented RNG */
    int create_inconsistent;         /* :39 */
    int create_inconsistent_border;  /* :40 */
    int out_equi_w, out_equi_h;      /* :46-47; 0 = no equirectangular output */
    int border_mode;                 /* fav_border of every warp (the reference's GPU path: FAV_BORDER_STN) */
} fav_vr_opts;
int fav_vr_create(fav_net* video_net, fav_net* image_net_or_null, int hplus, int wplus, const fav_vr_opts* opts, fav_vr** out);
void fav_vr_destroy(fav_vr* v);
/* one cube face.  frame: u8 [hplus][wplus][3]; backward_flo ([H][W][2] .flo payload) and cert_pgm (u8 [H][W]) are required
 * from the second frame on (i >= 7) and ignored before; out_rgb_f32 ([3][H][W], may be NULL) receives the stylised face */
int fav_vr_face(fav_vr* v, int i, const uint8_t* frame_rgb_hwc, const float* backward_flo, const uint8_t* cert_pgm,
                float* out_rgb_f32, fav_hipstream_t stream);
/* one cube face with the consistency check on the GPU: forward_flo = forward_{i-1}_[i].flo of this face; use_structure != 0 selects the
 * checker's 4-argument mode on this face's frame.  Faces that need no temporal certainty (i < 7, -create_inconsistent) ignore both flows
 * and behave exactly as fav_vr_face. */
int fav_vr_face_flow(fav_vr* v, int i, const uint8_t* frame_rgb_hwc, const float* backward_flo, const float* forward_flo,
                     int use_structure, float* out_rgb_f32, fav_hipstream_t stream);
/* optional look-ahead, event-ordered: start face i's mask on a side stream owned by the fav_vr (a mask depends on that face's frame and
 * flows only).  The next fav_vr_face_flow with the same i, pointers and mode consumes it; anything else discards it.  At most six
 * masks are pending, one per face of a frame (a second look-ahead for the same position of the frame replaces the first); the inputs
 * must stay unchanged until the face that consumes the mask has been enqueued.  A face that needs no temporal certainty: no-op. */
int fav_vr_prefetch_mask(fav_vr* v, int i, const uint8_t* frame_rgb_hwc, const float* backward_flo, const float* forward_flo,
                         int use_structure, fav_hipstream_t stream);
/* device pointer of the last mask fav_vr_face_flow computed (u8 [hplus][wplus], before the border max and the min filter) -- tests */
const uint8_t* fav_vr_last_mask(const fav_vr* v);
/* after the sixth face of a frame: post-blend (the blended faces become the next frame's warp sources), median filter,
 * equirectangular image (u8 [out_equi_h][out_equi_w][3]) and / or cube-map strip (u8 [cube_h][cube_w][3]); either may be NULL */
int fav_vr_finish_frame(fav_vr* v, uint8_t* equi_rgb8_hwc, uint8_t* cubemap_rgb8_hwc, fav_hipstream_t stream);
int fav_vr_output_sizes(const fav_vr* v, int* equi_w, int* equi_h, int* cube_w, int* cube_h, int* filtered_w, int* filtered_h);
/* float views for tests: which = 0 this frame's raw face k, 1 blended face k, 2 median-filtered face k, 3 equirectangular
 * image, 4 cube-map strip, 5 the certainty plane of the last face after border max and erosion ([hplus][wplus]; k ignored)
 * (device to device copy); 6 the border sum and 7 the prior of the last face ([3][hplus][wplus]; k ignored): fav_vr_state.h */
int fav_vr_get_f32(const fav_vr* v, int which, int k, float* out_dev, fav_hipstream_t stream);
/* the static maps, computed on the host (no device needed): kind 0..3 = perspective map left/right/top/bottom
 * ([2][hplus][wplus], `overlap` = the crop along that axis), 4 = cube->equirectangular map ([2][out_h][out_w]) */
int fav_vr_map_host(int kind, int hplus, int wplus, int overlap, int median_filter, int out_w, int out_h, float* out_host);
/* The transform stage: one equirectangular frame (u8 [equi_h][equi_w][3]) -> the six expanded cube faces (u8 [hplus][wplus][3] each) the
 * calls above take.  Stands in for transformVRVideo.sh's `ffmpeg -vf transform360=...:cube_edge_length=768:expand_coef=1.2` (a filter
 * that stock ffmpeg does not have).  The geometry is the inverse of the map of kind 4 above (median_filter 0) on the strip of
 * fast_artistic_video_vr.lua:543 -- faces[k] is processing position k = strip segment k, segments 4 and 5 rotated by 180 degrees -- on the
 * inner (hplus - overlap_h) x (wplus - overlap_w) of a face, continued over the overlap margin by the same pinhole projection: a face
 * spans tan = +-wplus / (wplus - overlap_w) (768 / 128: +-1.2).  Pixel index i of the frame is phi = 2 pi i / equi_w, row j is
 * theta = pi (1 - j / equi_h).  An output pixel is the mean of supersample^2 (1..4) Catmull-Rom bicubic samples on the regular grid of
 * sub-pixel centres, columns wrapping modulo equi_w, rows clamped; fp32; the u8 result is clamp(floor(v + 0.5), 0, 255) and the optional
 * fp32 planes ([hplus][wplus][3], 0..255 units) hold v.  This is NOT transform360's Lanczos-4 + low-pass filter; its quality against it
 * is unmeasured.  faces_rgb_hwc / faces_f32_or_null: HOST arrays of six device pointers (the second, or any entry of it, may be NULL).
 * One launch; allocates nothing, does not synchronise. */
int fav_vr_equi_to_faces_rgb8(const uint8_t* equi_rgb_hwc, int equi_w, int equi_h, int hplus, int wplus, int overlap_w, int overlap_h,
                              int supersample, uint8_t* const* faces_rgb_hwc, float* const* faces_f32_or_null, fav_hipstream_t stream);

/* ---- host-side formats (A1, A9) ----------------------------------------------------------------
 * .flo: flowFileLoader.lua:14-34 / consistencyChecker.cpp:16-36 (tag read, not validated);
 * P6/P5 8-bit binary PNM; PNG writer (RGB8, zlib).  Buffers are malloc'ed; free with fav_free_host. */
int fav_read_flo_host(const char* path, float** uv_out, int* W, int* H);
int fav_read_pnm_host(const char* path, uint8_t** data_out, int* W, int* H, int* channels);
/* the same readers into a caller-provided (e.g. pinned) buffer: no allocation, FAV_EINVAL if the payload does not fit */
int fav_read_flo_into_host(const char* path, float* uv_buf, size_t capacity_floats, int* W, int* H);
int fav_read_pnm_into_host(const char* path, uint8_t* buf, size_t capacity_bytes, int* W, int* H, int* channels);
int fav_write_pgm_host(const char* path, const uint8_t* data, int W, int H);
int fav_write_png_rgb8_host(const char* path, const uint8_t* rgb_hwc, int W, int H, int zlib_level);
void fav_free_host(void* p);

/* ---- A9 on the GPU: image.save("<prefix>-%05d.png", img) (fast_artistic_video.lua:160-170) -----------------------------------
 * The BYTES OF THE PNG FILE are produced on the device (Sub filter; one deflate block per image row -- run-length matches, the
 * cheapest of twelve ready-made Huffman codes / the fixed code / stored, by exact bit count -- re-aligned by an empty stored block;
 * Adler-32 and CRC-32 combined from per-row parts: csrc/kernels_png.hip, csrc/png_tables.cpp), so the host only write()s them: the
 * zlib path above costs ~25 ms per 1280x720 frame and core.  The files decode to exactly the bytes fav_stream_* writes to
 * out_rgb8_hwc (clamp to [0,1], x255, truncate); sizes are within a few per cent of zlib's level-1 run-length mode on image rows.
 *   png_out        device-ACCESSIBLE memory of fav_png_capacity(W, H) bytes, 4-byte aligned: device memory or host-mapped pinned
 *                  memory (hipHostMalloc: the packed bytes then cross PCIe once and are complete when the stream reaches the point
 *                  after the call -- use an event WITH the system-scope fence);
 *   png_bytes_out  device-accessible uint32: the file size;
 *   workspace      fav_png_workspace_bytes(W, H) bytes of device memory, 16-byte aligned, owned by the caller, private to the call
 *                  until the stream has passed it.
 * fav_png_encode_rgb8: rgb_hwc = u8 [H][W][3];  fav_png_encode_f32: planar float RGB [3][H][W] (what fav_stream_get_state returns),
 * quantisation fused.  Width <= 9000; any height whose file stays below 4 GiB.  rgb_hwc needs no padding or alignment:
 * nothing outside its H*W*3 bytes is read. */
size_t fav_png_capacity(int W, int H);
size_t fav_png_workspace_bytes(int W, int H);
int fav_png_encode_rgb8(const uint8_t* rgb_hwc, int W, int H, void* png_out, size_t capacity, uint32_t* png_bytes_out,
                        void* workspace, size_t workspace_bytes, fav_hipstream_t stream);
int fav_png_encode_f32(const float* rgb_planar, int W, int H, void* png_out, size_t capacity, uint32_t* png_bytes_out,
                       void* workspace, size_t workspace_bytes, fav_hipstream_t stream);
/* host-only (no device needed): the encoder's Huffman codes, for tools that restate its bit layout (oracle/png_model.py).
 * count tables of table_bytes bytes each: uint32 sym[277] = (code length << 16) | bit-reversed code; uint32 hdr[40] = the
 * dynamic-block header behind BFINAL / BTYPE, LSB first; uint32 hdr_bits, btype, dist_len, dist_code.  The last table is the
 * fixed code of RFC 1951 3.2.6.  out_host may be NULL to query count and table_bytes. */
int fav_png_tables_host(void* out_host, size_t capacity, int* count, int* table_bytes);
/* host-only (no device needed): crc32(A || B) from crc32(A), crc32(B) and |B| in bytes, by the table scheme the encoder's kernels use
 * to raise a row's CRC to its position in the IDAT chunk (any 32-bit length) -- lets the CPU suite pin it against zlib */
uint32_t fav_png_crc32_combine_host(uint32_t crc_a, uint32_t crc_b, uint32_t len_b);
/* the stream's current stylised frame (the recurrent state) as a PNG file, with the stream's own workspace */
int fav_stream_encode_png(fav_stream* s, void* png_out, size_t capacity, uint32_t* png_bytes_out, fav_hipstream_t stream);
/* the same file, produced NEXT TO whatever `stream` is given afterwards (normally the next frame's network: the encoder's short kernels
 * fill the tails of its grids instead of standing in front of it): enqueued on a queue the fav_stream owns, behind everything `stream`
 * holds at the time of the call.  The stream's state is double-buffered from the first such call on -- the next frame is written
 * next to the one being encoded, and the frame after it waits (on the device) for the encoder of the buffer it returns to -- so the
 * fav_stream_* calls may follow immediately.  png_out / png_bytes_out are complete when *png_bytes_out (set it to 0 first; e.g.
 * host-mapped memory) becomes the file's size, or behind fav_stream_wait_png on a queue of the caller's.  One encode per frame;
 * successive encodes run in order.  Same bytes as fav_stream_encode_png.  From the first call on the stream's network(s) run the way they
 * do next to the look-ahead masks (a few CUs left to the side queue, no hand-off between co-resident blocks of the generic kernel): the
 * encoder shares the device with the following forward.  A forward that fails leaves the state at the last complete frame.
 * User: `fav_stylize -png_overlap 1` (measured: no gain over the default). */
int fav_stream_encode_png_async(fav_stream* s, void* png_out, size_t capacity, uint32_t* png_bytes_out, fav_hipstream_t stream);
/* makes `stream` wait (on the device) for the asynchronous encodes issued so far */
int fav_stream_wait_png(fav_stream* s, fav_hipstream_t stream);

/* ---- YUV4MPEG2 (Y4M) video streams: 8-bit YCbCr planes <-> RGB on the GPU ---------------------------------------------------------
 * Stands in for the first and the last stage of every driver of the reference (stylizeVideo_deepflow.sh: `ffmpeg -i video
 * frame_%05d.ppm` ... `ffmpeg -i out-%05d.png video`): with `ffmpeg -f yuv4mpegpipe` on either side of fav_stylize -input_y4m /
 * -output_y4m the frames travel through pipes as planes, and the conversion ffmpeg would do on the CPU runs here.
 * A frame is the Y4M payload: plane Y [H][W], then Cb, then Cr, contiguous, 8 bits per sample; the chroma planes are [H][W] for 4:4:4 and
 * [ceil(H/2)][ceil(W/2)] for 4:2:0 (odd sizes are legal: a missing partner is the replicated edge sample).  The arithmetic -- fp32, one
 * stated order of operations, restated by tests/util/yuv_model.py and matched byte for byte -- is in DESIGN.md, "Y4M in and out":
 * (Kr, Kb) of BT.601 / BT.709; limited range Y 16..235, C 16..240, or full range; bytes are floor(x + 0.5) clamped to [0, 255] (limited
 * input outside 16..235 is legal and simply clamped after conversion); 4:2:0 chroma is interpolated bilinearly on the way in and
 * averaged over 2 x 2 (centre siting) / filtered 1-2-1 along x and averaged over two rows (left siting) on the way out.
 * Device pointers, caller-owned buffers of fav_yuv_frame_bytes / W*H*3 bytes with no alignment requirement, nothing allocated, no
 * synchronisation, nothing outside the buffers read or written.  A size below 1 x 1 or above 2^28 pixels, a null pointer or a field of
 * the format outside its values: FAV_EINVAL. */
enum fav_yuv_chroma { FAV_YUV_420 = 0, FAV_YUV_444 = 1 };
enum fav_yuv_siting { FAV_YUV_SITING_CENTER = 0 /* C420jpeg */, FAV_YUV_SITING_LEFT = 1 /* C420mpeg2 */ };
enum fav_yuv_matrix { FAV_YUV_BT601 = 0, FAV_YUV_BT709 = 1 };
typedef struct fav_yuv_format { int chroma;   /* FAV_YUV_420 | FAV_YUV_444 */
                                int siting;   /* FAV_YUV_SITING_CENTER (C420jpeg) | FAV_YUV_SITING_LEFT (C420mpeg2); ignored for 444 */
                                int matrix;   /* FAV_YUV_BT601 | FAV_YUV_BT709 */
                                int full_range; } fav_yuv_format;
/* bytes of one frame's payload (0 with a message: bad size or format) */
size_t fav_yuv_frame_bytes(int W, int H, const fav_yuv_format* fmt_host);
/* planes -> [H][W][3] u8, the layout fav_stream_* takes as frame_rgb_hwc */
int fav_yuv_to_rgb8(const uint8_t* yuv, int W, int H, const fav_yuv_format* fmt_host, uint8_t* rgb_hwc, fav_hipstream_t stream);
/* [H][W][3] u8 -> planes */
int fav_rgb8_to_yuv(const uint8_t* rgb_hwc, int W, int H, const fav_yuv_format* fmt_host, uint8_t* yuv, fav_hipstream_t stream);
/* planar float RGB [3][H][W] (what fav_stream_get_state returns) -> planes, image.save's quantisation (clamp to [0,1], x255, truncate:
 * fav_png_encode_f32's) fused in front: the planes are the conversion of exactly the bytes the PNG would have held */
int fav_rgb_f32_to_yuv(const float* rgb_planar, int W, int H, const fav_yuv_format* fmt_host, uint8_t* yuv, fav_hipstream_t stream);
/* the stream's current stylised frame (the recurrent state, Ho x Wo) as planes.  yuv_out: device memory or host-mapped pinned memory
 * (complete when the stream reaches the point after the call -- use an event WITH the system-scope fence) of `capacity` >=
 * fav_yuv_frame_bytes(Wo, Ho, fmt) bytes; a smaller capacity is FAV_EINVAL and nothing is written. */
int fav_stream_encode_yuv(fav_stream* s, const fav_yuv_format* fmt_host, uint8_t* yuv_out, size_t capacity, fav_hipstream_t stream);
/* ---- original colours: the stylised frame's luminance on the input frame's colours -------------------------------------------------
 * Not in the reference: the luminance transfer of Gatys et al., "Preserving color in neural artistic style transfer", where a frame
 * leaves (fav_stylize -original_colors 1).  S = image.save's bytes of the stylised planes (clamp to [0, 1], x255, truncate: those of
 * fav_png_encode_f32), O = the original frame's bytes.  Per pixel, fp32, in this order:
 *   ys = (Kr Sr + Kg Sg) + Kb Sb;  yo = (Kr Or + Kg Og) + Kb Ob;  d = ys - yo;  Pc = clamp(floor((Oc + d) + 0.5), 0, 255) for c = R, G, B
 * with (Kr, Kb) of `matrix` (FAV_YUV_BT601 | FAV_YUV_BT709), Kg = 1 - Kr - Kb; no range scaling enters.  Restated by
 * tests/util/color_model.py and matched byte for byte ("Original colours").
 * fav_color_transfer_rgb8 writes the image P, [H][W][3] u8; fav_color_transfer_yuv writes the planes of P -- the bytes of
 * fav_rgb8_to_yuv(P, fmt), whose matrix is also the transfer's -- without P ever existing in memory.
 * The conventions of the YUV operators above: device pointers, caller-owned buffers (3*W*H floats, W*H*3 bytes, fav_yuv_frame_bytes), no
 * alignment requirement, nothing allocated, no synchronisation, nothing outside the buffers read or written; a null pointer, a size below
 * 1 x 1 or above 2^28 pixels, a matrix or a field of the format outside its values: FAV_EINVAL. */
int fav_color_transfer_rgb8(const float* stylised_rgb_planar, const uint8_t* original_rgb_hwc, int W, int H, int matrix,
                            uint8_t* out_rgb_hwc, fav_hipstream_t stream);
int fav_color_transfer_yuv(const float* stylised_rgb_planar, const uint8_t* original_rgb_hwc, int W, int H,
                           const fav_yuv_format* fmt_host, uint8_t* yuv, fav_hipstream_t stream);
/* the same for a stream's current stylised frame (the recurrent state, which is only read: fav_stream_get_state gives the same bits
 * before and after) and `frame_rgb_hwc`, normally the frame the stream has just consumed.  The stream's output size must be the frame's
 * (fav_stream_output_size == H x W, i.e. both multiples of 4 for the canonical network): otherwise FAV_EUNSUPPORTED with a message that
 * names both sizes, and nothing is written.
 * fav_stream_encode_png_colors writes P into a buffer the stream owns (allocated at first use, freed with the stream) and runs the RGB8
 * encoder of fav_png_encode_rgb8 on it with the stream's own workspace: png_out / capacity / png_bytes_out as for fav_stream_encode_png
 * (png_bytes_out may be host-mapped memory).  fav_stream_encode_yuv_colors is one launch: yuv_out / capacity as for fav_stream_encode_yuv. */
int fav_stream_encode_png_colors(fav_stream* s, const uint8_t* frame_rgb_hwc, int matrix, void* png_out, size_t capacity,
                                 uint32_t* png_bytes_out, fav_hipstream_t stream);
int fav_stream_encode_yuv_colors(fav_stream* s, const uint8_t* frame_rgb_hwc, const fav_yuv_format* fmt_host, uint8_t* yuv_out,
                                 size_t capacity, fav_hipstream_t stream);
/* The stream header of YUV4MPEG2, host-only (no device needed): the magic `YUV4MPEG2`, then space-separated tags in any order, ended by
 * '\n'; at most FAV_Y4M_MAX_HEADER bytes.  `line` holds the header up to or including the newline (len bytes).
 *   W, H   required;  F<num>:<den> and A<num>:<den> are kept (fps_den 0 / aspect_num -1: the tag was absent and is not written back)
 *   I      absent, Ip or I? (kept in `interlace` as 0, 'p', '?'); It, Ib, Im: FAV_EUNSUPPORTED
 *   C      absent, C420, C420jpeg: 4:2:0, centre siting; C420mpeg2: 4:2:0, left siting; C444; every other tag (C420paldv, C422, C420p10,
 *          C444alpha, Cmono, ...): FAV_EUNSUPPORTED with a message that names the tag
 *   X...   kept verbatim, in order, space-separated, in `xtags`; XCOLORRANGE=FULL / =LIMITED also sets fmt.full_range (default: limited)
 * Y4M carries no matrix: the parser sets BT.709 when H >= 720, else BT.601 (the usual player heuristic); the caller may override it.
 * Anything malformed (magic, a missing W or H, a number that is none, an unknown tag letter, too long): FAV_EINVAL.
 * The formatter writes `YUV4MPEG2 W H F I A C X...` and the newline into buf_host and returns the number of bytes (> 0), or a negative
 * fav_status.  The X tags are written as kept, except XCOLORRANGE, which is written from fmt.full_range: in place where the tag was, or
 * appended (=FULL only) where it was not.  Parsing what the formatter wrote gives the header back.
 * A frame is `FRAME`, optional parameters, '\n', then fav_yuv_frame_bytes bytes. */
#define FAV_Y4M_MAX_HEADER 1024
typedef struct fav_y4m_header { int W, H; int fps_num, fps_den; int aspect_num, aspect_den; int interlace; fav_yuv_format fmt;
                                char xtags[FAV_Y4M_MAX_HEADER]; } fav_y4m_header;
int fav_y4m_parse_header_host(const char* line, size_t len, fav_y4m_header* out);
int fav_y4m_format_header_host(const fav_y4m_header* h, char* buf_host, size_t capacity);

/* ---- scene changes: how much the picture changed between two frames -----------------------------------------------------------------
 * Not in the reference, which expects a video cut into scenes by hand; a stream on a pipe cannot be (fav_stylize -scene_cut).
 * A block-histogram distance in integer arithmetic, restated by tests/util/scene_model.py and matched for EQUALITY:
 *   luma Y = (77 R + 150 G + 29 B + 128) >> 8, bin = Y >> 3 (32 bins); 4 x 4 cells, cell (cx, cy) = x in [cx W/4, (cx+1) W/4),
 *   y in [cy H/4, (cy+1) H/4) with floor division; cell[cy*4+cx] = sum over bins |hist_prev - hist_cur|; total = sum over cells.
 * The score is total / (2 W H) in [0, 1]; the caller forms it (in double), the device result is the 17 integers.
 *   prev / cur     u8 [H][W][3] in device memory, no alignment or padding: nothing outside their W*H*3 bytes is read; prev == cur is
 *                  allowed (all zeros).  W, H >= 4 and W * H <= 2^28, anything else is FAV_EINVAL.
 *   workspace      fav_scene_change_workspace_bytes() bytes of device memory, 16-byte aligned, private to the call until the stream has
 *                  passed it; zeroed by the call itself.  Fewer bytes: FAV_EINVAL and nothing is enqueued.
 *   result         any device-accessible address, 4-byte aligned: device memory or host-mapped memory (complete when the stream reaches
 *                  the point after the call).
 * Asynchronous on `stream`; nothing is allocated. */
typedef struct fav_scene_change { uint32_t total; uint32_t cell[16]; } fav_scene_change;   /* cell[cy*4+cx] */
size_t fav_scene_change_workspace_bytes(void);
int fav_scene_change_rgb8(const uint8_t* prev_rgb_hwc, const uint8_t* cur_rgb_hwc, int W, int H,
                          void* workspace, size_t workspace_bytes, fav_scene_change* result, fav_hipstream_t stream);

#ifdef __cplusplus
}
#endif
/* 4:2:2 and 9- to 16-bit Y4M frames: one more record (fav_yuv_layout) and the entry points that take it */
#include "fav_yuv.h"
/* long-term priors: a stream's history and the entries that merge the priors of several distances (fav_stylize -long_term) */
#include "fav_long_term.h"
/* writing a fav_vr's faces (the counterpart of fav_vr_get_f32): tests of the post-processing, resuming a 360-degree run */
#include "fav_vr_state.h"
#endif /* FAV_H */
