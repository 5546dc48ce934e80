#ifndef FAV_VR_STATE_H
#define FAV_VR_STATE_H
#include "fav.h"
#ifdef __cplusplus
extern "C" {
#endif

/* fav_vr_state.h -- writing the faces a fav_vr holds (the counterpart of fav_vr_get_f32) and reading what the last face's network was
 * given (below).  Included by fav.h, whose types it uses.
 *
 * Faces otherwise reach a fav_vr through the network only.  This entry puts them in directly: a test chooses what the post-processing
 * of fav_vr_finish_frame (post-blend, median filter, strips, quantisation) works on, and a 360-degree run that was interrupted is
 * resumed from the blended faces of its last finished frame (which = 1: they are the only state the next frame reads).
 *
 *   which = 0   this frame's raw face k (planar f32 [3][hplus][wplus], device memory), marked present: after all six,
 *               fav_vr_finish_frame runs as it does after six fav_vr_face calls, and a later face of the frame finds face k in place.
 *   which = 1   blended face k of the finished frame.  Once all six have been set since fav_vr_create or since the last
 *               fav_vr_finish_frame, the handle counts as having a previous frame (faces i >= 7 are accepted).
 * Any other `which`, a null pointer or k outside 0..5: FAV_EINVAL with a message, nothing is written.
 * One device-to-device copy on `stream`, no synchronisation, no allocation; in_dev must stay unchanged until the stream has passed it. */
int fav_vr_set_f32(fav_vr* v, int which, int k, const float* in_dev, fav_hipstream_t stream);

/* What the network of the last face read, stage by stage -- copies for tests, nothing on the frame path changes.
 *
 * fav_vr_get_f32, declared in fav.h, has two more kinds, both planar f32 [3][hplus][wplus], k ignored:
 *   which = 6   the border sum of the last fav_vr_face / fav_vr_face_flow call: the neighbours' faces, rotated, warped through the static
 *               perspective maps and summed (fast_artistic_video_vr.lua:248-272).  All zeros for mode 0 and under create_inconsistent_border.
 *   which = 7   the prior that face's input was assembled from: the border sum (first frame, -create_inconsistent), the flow-warped
 *               previous blended face (mode 0 of a later frame) or the blend of the two (:275-294).
 * Both are FAV_EINVAL with a message that names the kind, and write nothing, unless the last face call on the handle was a face with a
 * prior (not a single image, :304-310).  fav_vr_finish_frame sums its borders in the same buffer: after it kind 6 is refused, and kind 7
 * where the prior was the border sum itself.
 *
 * fav_vr_get_padded_input_f32: the last face's input as the network reads it, [hplus + 2 pad][wplus + 2 pad][8] (reflection padding of the
 * video model, eighth channel zero) -- the handle's own buffer, single images included.  FAV_EINVAL before the first face.
 * One device-to-device copy on `stream` each, no synchronisation, no allocation. */
int fav_vr_get_padded_input_f32(const fav_vr* v, float* out_dev, fav_hipstream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FAV_VR_STATE_H */
