/* fav_yuv.h -- YUV4MPEG2 frames of every layout fav_stylize takes: 4:2:0, 4:2:2 and 4:4:4 at 8, 9, 10, 12, 14 or 16 bits per sample.
 *
 * include/fav.h's YUV operators (fav_yuv_to_rgb8, ...) and its fav_yuv_format / fav_y4m_header cover 8-bit 4:2:0 and 4:4:4; those
 * records are caller-allocated and cannot grow, so they stay as they are and this header adds ONE self-describing record, fav_yuv_layout,
 * and one set of entry points that take it.  Phone and camera footage is 10-bit 4:2:0 (`C420p10`), broadcast and ProRes footage 4:2:2
 * (`C422`, `C422p10`): with these entry points such a stream goes through fav_stylize -input_y4m / -output_y4m as it is.
 *
 * A frame is the Y4M payload: plane Y [H][W], then Cb, then Cr, contiguous.  The chroma planes are [H][W] for 4:4:4, [H][ceil(W/2)] for
 * 4:2:2 and [ceil(H/2)][ceil(W/2)] for 4:2:0 (odd sizes are legal: a missing partner is the replicated edge sample).  A sample is one
 * byte at depth 8; otherwise it is two bytes, little-endian, with the value in the low `depth` bits -- which is what ffmpeg's
 * yuv4xxpNNle pipes are [recalled: ffmpeg is not on the project's machines].  An input sample is taken as the 16-bit number it is: no
 * masking, values above 2^depth - 1 are legal and simply clamped after conversion.
 *
 * Arithmetic: fp32, one stated order of operations, restated by tests/util/yuv_layout_model.py and matched sample for sample; DESIGN.md,
 * "Y4M in and out".  It is the arithmetic of fav.h's operators with the depth D in the constants, each formed in double and rounded once:
 *   m = 2^(D-8), q = (2^D - 1)/255;  limited range SY = (219/255) m, OY = 16 m, SC = (224/255) m;  full range SY = SC = q, OY = 0;
 *   OC = 2^(D-1)
 *   encode  y = (Kr R + Kg G) + Kb B;  Y = y SY + OY;  Cb = (B - y) (SC / (2 (1 - Kb))) + OC;  Cr = (R - y) (SC / (2 (1 - Kr))) + OC
 *   decode  y = (Y - OY) (1/SY);  cb = Cb - OC;  cr = Cr - OC;  R = y + kR cr;  B = y + kB cb;  G = (y - kGr cr) - kGb cb
 *   samples are floor(x + 0.5) clamped to [0, 2^D - 1], RGB bytes to [0, 255]
 * At D = 8 every constant is that of fav.h's operators, and for 4:2:0 and 4:4:4 the entry points below return those operators' bytes.
 * 4:2:0 interpolates and reduces as fav.h says, at every depth (the weights stay exact in fp32 on 16-bit samples).  4:2:2 is the
 * horizontal rule of each siting with no vertical step.  In: centre siting weighs neighbours 1/4 : 3/4; left siting gives column 2j the
 * sample C[j] and column 2j+1 the value 0.5 (C[j] + C[j+1]); indices clamped.  Out: the UNQUANTISED chroma is reduced, then quantised;
 * centre siting (c0 + c1) / 2, left siting ((l + r) + (c + c)) / 4 at the even column with neighbours clamped to the image.
 *
 * The fp32 source (fav_rgb_f32_to_yuv_layout, fav_stream_encode_yuv_layout) differs by depth, on purpose:
 *   depth 8    image.save's quantisation (clamp to [0, 1], x255, TRUNCATE) stands in front of the matrix exactly as in
 *              fav_rgb_f32_to_yuv: the planes are the conversion of the bytes the PNG would have held, both output routes show one image
 *   depth > 8  the floats enter UNQUANTISED: R = clamp(x, 0, 1) * 255, no truncation; the only rounding is the one to the sample.  That
 *              is the point of a deep output: a 10-bit encoder behind the pipe receives more than the 8 bits of the PNG.
 *
 * Conventions: those of fav.h's YUV operators.  Device pointers, caller-owned buffers of fav_yuv_layout_frame_bytes bytes for the planes
 * and W*H*3 bytes for the RGB image with NO alignment requirement (16-bit planes may start at an odd address), nothing allocated, no
 * synchronisation, nothing outside the buffers read or written.  Sizes 1 x 1 ... 2^28 pixels.  A null pointer, a size outside that or a
 * field of the layout outside its values is FAV_EINVAL with a message that names the field. */
#ifndef FAV_YUV_H
#define FAV_YUV_H
#include "fav.h"
#ifdef __cplusplus
extern "C" {
#endif

enum { FAV_YUV_422 = 2 };                     /* next to FAV_YUV_420 = 0, FAV_YUV_444 = 1 */
typedef struct fav_yuv_layout { uint32_t struct_bytes;   /* sizeof(fav_yuv_layout): checked, FAV_EINVAL otherwise */
                                int chroma;      /* FAV_YUV_420 | FAV_YUV_444 | FAV_YUV_422 */
                                int siting;      /* FAV_YUV_SITING_CENTER | FAV_YUV_SITING_LEFT; 420 and 422 read it (422: along x only); 444 ignores it */
                                int matrix;      /* FAV_YUV_BT601 | FAV_YUV_BT709 */
                                int full_range;
                                int depth; } fav_yuv_layout;  /* 8, 9, 10, 12, 14 or 16 bits per sample */

/* bytes of one frame's payload (0 with a message: bad size or field).  No device needed. */
size_t fav_yuv_layout_frame_bytes(int W, int H, const fav_yuv_layout* layout_host);
/* planes of any layout -> [H][W][3] u8, the layout fav_stream_* takes as frame_rgb_hwc */
int fav_yuv_layout_to_rgb8(const void* yuv, int W, int H, const fav_yuv_layout* layout_host, uint8_t* rgb_hwc, fav_hipstream_t stream);
/* [H][W][3] u8 -> planes */
int fav_rgb8_to_yuv_layout(const uint8_t* rgb_hwc, int W, int H, const fav_yuv_layout* layout_host, void* yuv, fav_hipstream_t stream);
/* planar float RGB [3][H][W] -> planes; depth 8 truncates like image.save first, a deeper layout takes the floats unquantised (above) */
int fav_rgb_f32_to_yuv_layout(const float* rgb_planar, int W, int H, const fav_yuv_layout* layout_host, void* yuv, fav_hipstream_t stream);
/* the stream's current stylised frame (the recurrent state, Ho x Wo, which is only read) as planes, by the rule of
 * fav_rgb_f32_to_yuv_layout.  yuv_out / capacity as for fav_stream_encode_yuv: device or host-mapped pinned memory of `capacity` >=
 * fav_yuv_layout_frame_bytes(Wo, Ho, layout) bytes; a smaller capacity is FAV_EINVAL and nothing is written. */
int fav_stream_encode_yuv_layout(fav_stream* s, const fav_yuv_layout* layout_host, void* yuv_out, size_t capacity, fav_hipstream_t stream);

/* The stream header, host-only: the grammar of fav_y4m_parse_header_host / fav_y4m_format_header_host (fav.h) with more C tags.
 *   C      absent, C420, C420jpeg: 4:2:0, centre siting; C420mpeg2: 4:2:0, left siting; C444; C422: 4:2:2, LEFT siting (MPEG-2 4:2:2 is
 *          co-sited horizontally [recalled]); C420pN, C422pN, C444pN with N in 9, 10, 12, 14, 16: N bits, 420pN centre, 422pN left siting.
 *          C420paldv, C411, Cmono..., C444alpha, any other depth: FAV_EUNSUPPORTED with a message that names the tag.
 * Everything else -- W, H, F, A, I, the X tags, XCOLORRANGE, the matrix chosen from H, FAV_EINVAL for anything malformed -- is as there: a
 * header that parser accepts gives the same fields here, and the same formatted line.
 * The formatter writes the tag that the parser reads back as (chroma, siting, depth).  The grammar has no tag for 4:2:2 with centre
 * siting, nor for left-sited 4:2:0 deeper than 8 bits: those are FAV_EUNSUPPORTED.
 * A frame is `FRAME`, optional parameters, '\n', then fav_yuv_layout_frame_bytes bytes. */
typedef struct fav_y4m_stream_header { int W, H; int fps_num, fps_den; int aspect_num, aspect_den; int interlace; fav_yuv_layout layout;
                                       char xtags[FAV_Y4M_MAX_HEADER]; } fav_y4m_stream_header;
int fav_y4m_parse_stream_header_host(const char* line, size_t len, fav_y4m_stream_header* out);
int fav_y4m_format_stream_header_host(const fav_y4m_stream_header* h, char* buf_host, size_t capacity);

#ifdef __cplusplus
}
#endif
#endif /* FAV_YUV_H */
