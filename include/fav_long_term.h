#ifndef FAV_LONG_TERM_H
#define FAV_LONG_TERM_H
#include "fav.h"
#ifdef __cplusplus
extern "C" {
#endif

/* fav_long_term.h -- long-term priors (fav_stylize -long_term; DESIGN.md, "Long-term priors").  Included by fav.h, whose types it uses.
 *
 * Ruder, Dosovitskiy, Brox, "Artistic style transfer for videos" (2016), section 4.2: besides frame i - 1 the stylised frames i - d of
 * a few more distances d are warped to frame i, and every pixel takes the NEAREST frame in which it was visible,
 *     w_k = max(c_k - sum_{j<k} c_j, 0),   prior = sum_k w_k * pre(warp_k),   C = sum_k w_k        (c_k: eroded certainty of d_k)
 * so that background uncovered behind a moving object is continued from before it was covered instead of being invented anew.  The
 * network, its weights and its 7-channel input are unchanged: only the prior planes and the certainty plane are better informed.
 * Off by default; without fav_stream_set_long_term every entry of fav.h does what it did, launch for launch.
 *
 * fav_long_term_input_f32: the merged input assembly alone (csrc/kernels_longterm.hip; restated by tests/util/long_term_model.py).
 * states / backward_flo / cert are HOST arrays of n (1..FAV_LONG_TERM_MAX) device pointers in ascending distance: [3][Hs][Ws] f32,
 * [H][W][2] f32 (.flo payload), [H][W] f32 eroded certainty in [0, 1].  in8_out: [H+2p][W+2p][8] f32 (p = pad, reflection folded in,
 * channel 7 zero); cert_out: the merged certainty C [H][W] f32, or NULL.  A prior whose weight is 0 at a pixel is not sampled there:
 * a non-finite flow of that distance leaves nothing behind.  With n = 1 the result is what the stream's own input assembly writes,
 * bit for bit.  fill_random / seed / index: the uniform-random fill under the merged certainty (index: the stream's frame counter).
 * Enqueues one launch; FAV_EINVAL (nothing launched) for n out of range, a null pointer, 0 > pad or pad >= H, W. */
#define FAV_LONG_TERM_MAX 4          /* distances per frame, distance 1 included */
#define FAV_LONG_TERM_MAX_DISTANCE 16
int fav_long_term_input_f32(const uint8_t* frame_rgb_hwc, int n, const float* const* states, int Hs, int Ws,
                            const float* const* backward_flo, const float* const* cert, int border,
                            int H, int W, int pad, int fill_random, unsigned seed, unsigned index,
                            float* in8_out, float* cert_out, fav_hipstream_t stream);
/* distances_host: n strictly ascending ints, distances_host[0] == 1, the last <= FAV_LONG_TERM_MAX_DISTANCE, n <= FAV_LONG_TERM_MAX;
 * n == 0 turns the feature off and frees its buffers.  Anything else: FAV_EINVAL with a message that names the value, the stream as it
 * was.  The call allocates -- here, not per frame -- the HISTORY, a ring of the last max-distance stylised frames [3][Ho][Wo] and input
 * frames [H][W][3] (device copies the stream owns), and one mask and certainty plane per distance; it starts the history empty but for
 * the current state, if there is one (as fav_stream_set_state would).
 *   History.  After every frame -- whichever fav_stream_* entry ran it -- the frame's bytes and its stylised state enter the ring (two
 *     device-to-device copies on the caller's queue).  fav_stream_first_frame and fav_stream_set_state EMPTY the ring first and then
 *     insert their own frame + state, or state (which has no frame): the first frame, a scene cut and -continue_with.  Frame i after a
 *     restart at r therefore uses exactly the distances d <= i - r; nothing from before the restart is ever warped in.
 *   fav_stream_long_term_available: how many of the configured distances, counted from the first, the history can serve now.
 *   Untouched entries.  Every fav_stream_next_frame_* of fav.h works on such a stream as before (distance 1 only) and feeds the history.
 *   Unchanged views.  fav_stream_last_mask stays the distance-1 mask; fav_stream_get_input_f32 / _padded_input_f32 show the MERGED
 *     input; fav_temporal_loss* keep measuring distance 1.
 *   Look-ahead.  The _lt calls do not use fav_stream_prefetch_mask; a look-ahead pending when one arrives is FAV_EINVAL, not a mix.
 *   Errors.  m < 1 or larger than what is available, a null pointer among the first m, a workspace that is too small, long-term priors
 *     off: FAV_EINVAL, and nothing is launched.
 * fav_stream_next_frame_flows_lt: the next frame with the flows given -- HOST arrays of m device pointers for the first m configured
 *   distances; backward_flo[k]: A = this frame, B = frame i - d_k; forward_flo[k] the other way.  Each distance gets the forward-backward
 *   check, the certainty options and the erosion of the stream's options (the 4-argument structure map depends on this frame alone and is
 *   computed once), then the merged assembly and the network.  With m = 1 the frame is fav_stream_next_frame_flow's, byte for byte.
 * fav_stream_next_frame_estimate_lt: the next frame from the frames alone -- ONE fav_flow_pairs_rgb8_ex3 call with n_pairs = the
 *   available distances whose history entry holds a frame (prev[k] = the history's frame i - d_k, cur[k] = this frame), then the call
 *   above.  At least distance 1 must hold a frame: right after fav_stream_set_state it does not, and that frame takes
 *   fav_stream_next_frame_estimate_ex3, which is given the previous frame.
 *   workspace: fav_stream_long_term_workspace_bytes(s, opts) bytes, 256-byte aligned (0 with a message: bad options, feature off): 2 n
 *   flow fields of F = H * W * 8 rounded up to 256 bytes -- backward_flo[k] at byte 2 k F, forward_flo[k] at (2 k + 1) F, where the
 *   caller may read them after the call -- followed by fav_flow_pairs_workspace_bytes_ex3(W, H, n, opts) bytes. */
int fav_stream_set_long_term(fav_stream* s, const int* distances_host, int n);
int fav_stream_long_term_available(const fav_stream* s);
int fav_stream_next_frame_flows_lt(fav_stream* s, const uint8_t* frame_rgb_hwc, int m,
                                   const float* const* backward_flo, const float* const* forward_flo,
                                   int use_structure, float* out_rgb_f32, uint8_t* out_rgb8_hwc, fav_hipstream_t stream);
size_t fav_stream_long_term_workspace_bytes(const fav_stream* s, const fav_flow_opts_ex3* opts_host);
int fav_stream_next_frame_estimate_lt(fav_stream* s, const uint8_t* frame_rgb_hwc, const fav_flow_opts_ex3* opts_host,
                                      int use_structure, void* workspace, size_t workspace_bytes,
                                      float* out_rgb_f32, uint8_t* out_rgb8_hwc, fav_hipstream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FAV_LONG_TERM_H */
