#ifndef FAV_VR_STATE_H
#define FAV_VR_STATE_H
#include "fav.h"
#ifdef __cplusplus
extern "C" {
#endif

/* fav_vr_state.h -- writing the faces a fav_vr holds: the counterpart of fav_vr_get_f32.  Included by fav.h, whose types it uses.
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

#ifdef __cplusplus
}
#endif
#endif /* FAV_VR_STATE_H */
