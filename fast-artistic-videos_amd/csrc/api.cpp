// api.cpp -- C ABI glue: error reporting, device check, operator-level entry points (A2, A3/A4, A5, A6/A7)
// and the host-side file formats (A1, A9).  See include/fav.h for the reference interfaces replaced.
#include <unistd.h>
#include <zlib.h>

#include <cctype>
#include <cstdlib>
#include <cstring>

#include "dev_owned.h"

#include <dlfcn.h>

namespace fav {

namespace {
struct Roctx { int (*push)(const char*) = nullptr; int (*pop)() = nullptr; };
const Roctx& roctx()
{
    static const Roctx r = [] {
        Roctx x;
        if (!getenv("FAV_ROCTX")) return x;
        for (const char* lib : {"librocprofiler-sdk-roctx.so", "librocprofiler-sdk-roctx.so.1", "libroctx64.so", "libroctx64.so.4"}) {
            if (void* h = dlopen(lib, RTLD_NOW | RTLD_GLOBAL)) {
                x.push = reinterpret_cast<int (*)(const char*)>(dlsym(h, "roctxRangePushA"));
                x.pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
                if (x.push && x.pop) return x;
                x = Roctx();
            }
        }
        return x;
    }();
    return r;
}
}  // namespace

bool TraceRange::enabled() { return roctx().push != nullptr; }
TraceRange::TraceRange(const char* name) : on(roctx().push != nullptr) { if (on) roctx().push(name); }
TraceRange::~TraceRange() { if (on) roctx().pop(); }


static thread_local char g_err[1024] = "";

void set_error(const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}

int hip_fail(hipError_t e, const char* what)
{
    set_error("HIP error %d (%s) in %s", (int)e, hipGetErrorString(e), what);
    return FAV_EHIP;
}

int ensure_device()
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        set_error("no HIP device available (%s): libfav has no CPU fallback", e == hipSuccess ? "0 devices" : hipGetErrorString(e));
        return FAV_ENODEVICE;
    }
    return FAV_OK;
}

}  // namespace fav

using namespace fav;

extern "C" const char* fav_last_error(void) { return g_err; }
extern "C" int fav_version(void) { return 100; }

extern "C" int fav_device_count(void)
{
    int rc = ensure_device();
    if (rc) return rc;
    int n = 0;
    (void)hipGetDeviceCount(&n);
    return n;
}

extern "C" int fav_warp_bdhw_f32(const float* img, const float* flow, float* out, int B, int C, int H, int W, int Ho, int Wo,
                                 int border_mode, fav_hipstream_t stream)
{
    // shape contract of BilinearSamplerBDHW.lua:26-42
    FAV_REQUIRE(img && flow && out, "fav_warp_bdhw_f32: null pointer");
    FAV_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0 && Ho > 0 && Wo > 0, "fav_warp_bdhw_f32: non-positive dimension");
    FAV_REQUIRE(border_mode == FAV_BORDER_STN || border_mode == FAV_BORDER_CPU, "fav_warp_bdhw_f32: unknown border mode %d", border_mode);
    int rc = ensure_device(); if (rc) return rc;
    return launch_warp(img, flow, out, B, C, H, W, Ho, Wo, border_mode, static_cast<hipStream_t>(stream));
}

extern "C" size_t fav_consistency_workspace_bytes(int W, int H, int with_structure)
{
    return with_structure ? structure_workspace_bytes(W, H) : 0;
}

extern "C" int fav_consistency_u8(const float* flow1_flo, const float* flow2_flo, const uint8_t* rgb_hwc, uint8_t* out, int W,
                                  int H, void* workspace, size_t workspace_bytes, fav_hipstream_t stream)
{
    FAV_REQUIRE(flow1_flo && flow2_flo && out && W > 0 && H > 0, "fav_consistency_u8: bad argument");
    int rc = ensure_device(); if (rc) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const float* structure = nullptr; const float* avg = nullptr;
    if (rgb_hwc) {
        rc = launch_structure(rgb_hwc, W, H, workspace, workspace_bytes, &structure, &avg, st);
        if (rc) return rc;
    }
    return launch_consistency(flow1_flo, flow2_flo, structure, avg, out, W, H, st);
}

// test / tool entry: the structure map of the 4-argument mode itself, in either launch form (see include/fav.h)
extern "C" int fav_structure_f32(const uint8_t* rgb_hwc, int W, int H, void* workspace, size_t workspace_bytes, float* structure_out,
                                 float* avg_out, int pack_cus, int q0, int* form_ran, fav_hipstream_t stream)
{
    FAV_REQUIRE(rgb_hwc && workspace && structure_out && avg_out && form_ran, "fav_structure_f32: null pointer");
    FAV_REQUIRE(W >= 2 && H >= 2 && (long long)W * H <= (1ll << 28), "fav_structure_f32: bad frame size %dx%d (both sides at least 2, at most 2^28 pixels)", W, H);
    FAV_REQUIRE(pack_cus >= 0 && pack_cus <= 4, "fav_structure_f32: pack_cus must be 0 (wide form) .. 4, not %d", pack_cus);
    FAV_REQUIRE(q0 >= 0 && q0 <= 7, "fav_structure_f32: q0 must be 0 .. 7, not %d", q0);
    FAV_REQUIRE(workspace_bytes >= structure_workspace_bytes(W, H), "fav_structure_f32: the workspace holds %zu bytes, fav_consistency_workspace_bytes(W, H, 1) is %zu",
                workspace_bytes, structure_workspace_bytes(W, H));
    int rc = ensure_device(); if (rc) return rc;
    return launch_structure_map(rgb_hwc, W, H, workspace, workspace_bytes, structure_out, avg_out, pack_cus, q0, form_ran, static_cast<hipStream_t>(stream));
}

extern "C" int fav_min_filter_f32(const float* cert, float* out, int H, int W, int r, fav_hipstream_t stream)
{
    FAV_REQUIRE(cert && out && H > 0 && W > 0 && r >= 1, "fav_min_filter_f32: bad argument");
    int rc = ensure_device(); if (rc) return rc;
    return launch_min_filter_f32(cert, out, H, W, r, static_cast<hipStream_t>(stream));
}

extern "C" int fav_scale_bicubic_f32(const float* src, float* dst, int C, int Hs, int Ws, int Hd, int Wd, fav_hipstream_t stream)
{
    FAV_REQUIRE(src && dst, "fav_scale_bicubic_f32: null pointer");
    FAV_REQUIRE(C > 0 && Hs > 0 && Ws > 0 && Hd > 0 && Wd > 0, "fav_scale_bicubic_f32: non-positive dimension");
    int rc = ensure_device(); if (rc) return rc;
    return launch_scale_planar(src, dst, C, Hs, Ws, Hd, Wd, static_cast<hipStream_t>(stream));
}

// ---- A9 on the GPU: the bytes of the PNG file (kernels_png.hip)
extern "C" size_t fav_png_capacity(int W, int H) { return (W > 0 && H > 0) ? png_capacity(W, H) : 0; }
extern "C" size_t fav_png_workspace_bytes(int W, int H) { return (W > 0 && H > 0) ? png_workspace_bytes(W, H) : 0; }

extern "C" uint32_t fav_png_crc32_combine_host(uint32_t crc_a, uint32_t crc_b, uint32_t len_b) { return png_crc32_combine_host(crc_a, crc_b, len_b); }

extern "C" int fav_png_encode_rgb8(const uint8_t* rgb_hwc, int W, int H, void* png_out, size_t capacity, uint32_t* png_bytes_out,
                                   void* workspace, size_t workspace_bytes, fav_hipstream_t stream)
{
    FAV_REQUIRE(rgb_hwc, "fav_png_encode_rgb8: null image");
    int rc = ensure_device(); if (rc) return rc;
    return launch_png_encode(rgb_hwc, nullptr, W, H, png_out, capacity, png_bytes_out, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}

extern "C" int fav_png_encode_f32(const float* rgb_planar, int W, int H, void* png_out, size_t capacity, uint32_t* png_bytes_out,
                                  void* workspace, size_t workspace_bytes, fav_hipstream_t stream)
{
    FAV_REQUIRE(rgb_planar, "fav_png_encode_f32: null image");
    int rc = ensure_device(); if (rc) return rc;
    return launch_png_encode(nullptr, rgb_planar, W, H, png_out, capacity, png_bytes_out, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}

// ---- YUV4MPEG2: 8-bit YCbCr planes <-> RGB (kernels_yuv.hip)
int fav::yuv_format_check(const char* who, int W, int H, const fav_yuv_format* f)
{
    FAV_REQUIRE(f, "%s: null format", who);
    FAV_REQUIRE(W > 0 && H > 0 && (long long)W * H <= (1ll << 28), "%s: bad frame size %dx%d", who, W, H);
    FAV_REQUIRE(f->chroma == FAV_YUV_420 || f->chroma == FAV_YUV_444, "%s: chroma must be 0 (4:2:0) or 1 (4:4:4), not %d", who, f->chroma);
    FAV_REQUIRE(f->chroma == FAV_YUV_444 || f->siting == FAV_YUV_SITING_CENTER || f->siting == FAV_YUV_SITING_LEFT,
                "%s: siting must be 0 (centre, C420jpeg) or 1 (left, C420mpeg2), not %d", who, f->siting);
    FAV_REQUIRE(f->matrix == FAV_YUV_BT601 || f->matrix == FAV_YUV_BT709, "%s: matrix must be 0 (BT.601) or 1 (BT.709), not %d", who, f->matrix);
    return FAV_OK;
}

extern "C" size_t fav_yuv_frame_bytes(int W, int H, const fav_yuv_format* fmt_host)
{
    return yuv_format_check("fav_yuv_frame_bytes", W, H, fmt_host) ? 0 : yuv_frame_bytes(W, H, *fmt_host);
}

extern "C" int fav_yuv_to_rgb8(const uint8_t* yuv, int W, int H, const fav_yuv_format* fmt_host, uint8_t* rgb_hwc, fav_hipstream_t stream)
{
    FAV_REQUIRE(yuv && rgb_hwc, "fav_yuv_to_rgb8: null pointer");
    int rc = yuv_format_check("fav_yuv_to_rgb8", W, H, fmt_host); if (rc) return rc;
    rc = ensure_device(); if (rc) return rc;
    return launch_yuv_to_rgb8(yuv, W, H, *fmt_host, rgb_hwc, static_cast<hipStream_t>(stream));
}

extern "C" int fav_rgb8_to_yuv(const uint8_t* rgb_hwc, int W, int H, const fav_yuv_format* fmt_host, uint8_t* yuv, fav_hipstream_t stream)
{
    FAV_REQUIRE(rgb_hwc && yuv, "fav_rgb8_to_yuv: null pointer");
    int rc = yuv_format_check("fav_rgb8_to_yuv", W, H, fmt_host); if (rc) return rc;
    rc = ensure_device(); if (rc) return rc;
    return launch_rgb_to_yuv(rgb_hwc, nullptr, W, H, *fmt_host, yuv, static_cast<hipStream_t>(stream));
}

extern "C" int fav_rgb_f32_to_yuv(const float* rgb_planar, int W, int H, const fav_yuv_format* fmt_host, uint8_t* yuv, fav_hipstream_t stream)
{
    FAV_REQUIRE(rgb_planar && yuv, "fav_rgb_f32_to_yuv: null pointer");
    int rc = yuv_format_check("fav_rgb_f32_to_yuv", W, H, fmt_host); if (rc) return rc;
    rc = ensure_device(); if (rc) return rc;
    return launch_rgb_to_yuv(nullptr, rgb_planar, W, H, *fmt_host, yuv, static_cast<hipStream_t>(stream));
}

// ---- every layout of include/fav_yuv.h: 4:2:0, 4:2:2, 4:4:4 at 8 .. 16 bits (kernels_yuv_layout.hip)
static bool yuv_depth_ok(int d) { return d == 8 || d == 9 || d == 10 || d == 12 || d == 14 || d == 16; }

int fav::yuv_layout_check(const char* who, int W, int H, const fav_yuv_layout* l)
{
    FAV_REQUIRE(l, "%s: null layout", who);
    FAV_REQUIRE(l->struct_bytes == sizeof(fav_yuv_layout), "%s: struct_bytes must be %zu (sizeof(fav_yuv_layout)), not %u", who, sizeof(fav_yuv_layout), l->struct_bytes);
    FAV_REQUIRE(W > 0 && H > 0 && (long long)W * H <= (1ll << 28), "%s: bad frame size %dx%d", who, W, H);
    FAV_REQUIRE(l->chroma == FAV_YUV_420 || l->chroma == FAV_YUV_444 || l->chroma == FAV_YUV_422, "%s: chroma must be 0 (4:2:0), 1 (4:4:4) or 2 (4:2:2), not %d", who, l->chroma);
    FAV_REQUIRE(l->chroma == FAV_YUV_444 || l->siting == FAV_YUV_SITING_CENTER || l->siting == FAV_YUV_SITING_LEFT,
                "%s: siting must be 0 (centre) or 1 (left), not %d", who, l->siting);
    FAV_REQUIRE(l->matrix == FAV_YUV_BT601 || l->matrix == FAV_YUV_BT709, "%s: matrix must be 0 (BT.601) or 1 (BT.709), not %d", who, l->matrix);
    FAV_REQUIRE(yuv_depth_ok(l->depth), "%s: depth must be 8, 9, 10, 12, 14 or 16, not %d", who, l->depth);
    return FAV_OK;
}

extern "C" size_t fav_yuv_layout_frame_bytes(int W, int H, const fav_yuv_layout* layout_host)
{
    return yuv_layout_check("fav_yuv_layout_frame_bytes", W, H, layout_host) ? 0 : yuv_layout_frame_bytes(W, H, *layout_host);
}

extern "C" int fav_yuv_layout_to_rgb8(const void* yuv, int W, int H, const fav_yuv_layout* layout_host, uint8_t* rgb_hwc, fav_hipstream_t stream)
{
    FAV_REQUIRE(yuv && rgb_hwc, "fav_yuv_layout_to_rgb8: null pointer");
    int rc = yuv_layout_check("fav_yuv_layout_to_rgb8", W, H, layout_host); if (rc) return rc;
    rc = ensure_device(); if (rc) return rc;
    return launch_yuv_layout_to_rgb8(yuv, W, H, *layout_host, rgb_hwc, static_cast<hipStream_t>(stream));
}

extern "C" int fav_rgb8_to_yuv_layout(const uint8_t* rgb_hwc, int W, int H, const fav_yuv_layout* layout_host, void* yuv, fav_hipstream_t stream)
{
    FAV_REQUIRE(rgb_hwc && yuv, "fav_rgb8_to_yuv_layout: null pointer");
    int rc = yuv_layout_check("fav_rgb8_to_yuv_layout", W, H, layout_host); if (rc) return rc;
    rc = ensure_device(); if (rc) return rc;
    return launch_rgb_to_yuv_layout(rgb_hwc, nullptr, W, H, *layout_host, yuv, static_cast<hipStream_t>(stream));
}

extern "C" int fav_rgb_f32_to_yuv_layout(const float* rgb_planar, int W, int H, const fav_yuv_layout* layout_host, void* yuv, fav_hipstream_t stream)
{
    FAV_REQUIRE(rgb_planar && yuv, "fav_rgb_f32_to_yuv_layout: null pointer");
    int rc = yuv_layout_check("fav_rgb_f32_to_yuv_layout", W, H, layout_host); if (rc) return rc;
    rc = ensure_device(); if (rc) return rc;
    return launch_rgb_to_yuv_layout(nullptr, rgb_planar, W, H, *layout_host, yuv, static_cast<hipStream_t>(stream));
}

// ---- original colours: the stylised frame's luminance on the original frame's colours (kernels_color.hip)
extern "C" int fav_color_transfer_rgb8(const float* stylised_rgb_planar, const uint8_t* original_rgb_hwc, int W, int H, int matrix,
                                       uint8_t* out_rgb_hwc, fav_hipstream_t stream)
{
    FAV_REQUIRE(stylised_rgb_planar && original_rgb_hwc && out_rgb_hwc, "fav_color_transfer_rgb8: null pointer");
    const fav_yuv_format f{FAV_YUV_444, FAV_YUV_SITING_CENTER, matrix, 1};      // (size and matrix: the YUV operators' rules)
    int rc = yuv_format_check("fav_color_transfer_rgb8", W, H, &f); if (rc) return rc;
    rc = ensure_device(); if (rc) return rc;
    return launch_color_transfer_rgb8(stylised_rgb_planar, original_rgb_hwc, W, H, matrix, out_rgb_hwc, static_cast<hipStream_t>(stream));
}

extern "C" int fav_color_transfer_yuv(const float* stylised_rgb_planar, const uint8_t* original_rgb_hwc, int W, int H,
                                      const fav_yuv_format* fmt_host, uint8_t* yuv, fav_hipstream_t stream)
{
    FAV_REQUIRE(stylised_rgb_planar && original_rgb_hwc && yuv, "fav_color_transfer_yuv: null pointer");
    int rc = yuv_format_check("fav_color_transfer_yuv", W, H, fmt_host); if (rc) return rc;
    rc = ensure_device(); if (rc) return rc;
    return launch_color_transfer_yuv(stylised_rgb_planar, original_rgb_hwc, W, H, *fmt_host, yuv, static_cast<hipStream_t>(stream));
}

// ---- scene changes: the block-histogram distance of two frames (kernels_scene.hip)
extern "C" size_t fav_scene_change_workspace_bytes(void) { return scene_change_workspace_bytes(); }

extern "C" int fav_scene_change_rgb8(const uint8_t* prev_rgb_hwc, const uint8_t* cur_rgb_hwc, int W, int H, void* workspace, size_t workspace_bytes,
                                     fav_scene_change* result, fav_hipstream_t stream)
{
    FAV_REQUIRE(prev_rgb_hwc && cur_rgb_hwc && workspace && result, "fav_scene_change_rgb8: null pointer");
    FAV_REQUIRE(W >= 4 && H >= 4 && (long long)W * H <= (1ll << 28), "fav_scene_change_rgb8: bad frame size %dx%d (4 x 4 cells: both sides at least 4, at most 2^28 pixels)", W, H);
    FAV_REQUIRE(workspace_bytes >= scene_change_workspace_bytes(), "fav_scene_change_rgb8: the workspace holds %zu bytes, fav_scene_change_workspace_bytes() is %zu",
                workspace_bytes, scene_change_workspace_bytes());
    FAV_REQUIRE(((uintptr_t)workspace & 15u) == 0 && ((uintptr_t)result & 3u) == 0, "fav_scene_change_rgb8: the workspace must be 16-byte aligned, the result 4-byte aligned");
    int rc = ensure_device(); if (rc) return rc;
    return launch_scene_change(prev_rgb_hwc, cur_rgb_hwc, W, H, workspace, result, static_cast<hipStream_t>(stream));
}

extern "C" int fav_assemble_input_f32(const float* frame_rgb, const float* warped_rgb, const float* cert, float* in7, int H,
                                      int W, fav_hipstream_t stream)
{
    FAV_REQUIRE(frame_rgb && in7 && H > 0 && W > 0, "fav_assemble_input_f32: bad argument");
    FAV_REQUIRE((warped_rgb == nullptr) == (cert == nullptr), "fav_assemble_input_f32: warped_rgb and cert must both be given or both be NULL");
    int rc = ensure_device(); if (rc) return rc;
    return launch_assemble(frame_rgb, warped_rgb, cert, in7, H, W, static_cast<hipStream_t>(stream));
}

// the merged input assembly of the long-term priors on its own (kernels_longterm.hip)
extern "C" int fav_long_term_input_f32(const uint8_t* frame_rgb_hwc, int n, const float* const* states, int Hs, int Ws,
                                       const float* const* backward_flo, const float* const* cert, int border, int H, int W, int pad,
                                       int fill_random, unsigned seed, unsigned index, float* in8_out, float* cert_out, fav_hipstream_t stream)
{
    FAV_REQUIRE(n >= 1 && n <= FAV_LONG_TERM_MAX, "fav_long_term_input_f32: %d priors (1..%d)", n, FAV_LONG_TERM_MAX);
    FAV_REQUIRE(frame_rgb_hwc && states && backward_flo && cert && in8_out, "fav_long_term_input_f32: null pointer");
    FAV_REQUIRE(H > 0 && W > 0 && Hs > 0 && Ws > 0 && pad >= 0 && pad < H && pad < W, "fav_long_term_input_f32: needs H, W, Hs, Ws > 0 and 0 <= pad < H, W (pad %d, %dx%d)", pad, W, H);
    FAV_REQUIRE(border == FAV_BORDER_STN || border == FAV_BORDER_CPU, "fav_long_term_input_f32: border mode %d", border);
    for (int k = 0; k < n; ++k)
        FAV_REQUIRE(states[k] && backward_flo[k] && cert[k], "fav_long_term_input_f32: null pointer for prior %d", k);
    int rc = ensure_device(); if (rc) return rc;
    return launch_longterm_prep(frame_rgb_hwc, n, states, Hs, Ws, backward_flo, cert, border, H, W, pad, in8_out, cert_out,
                                static_cast<hipStream_t>(stream), fill_random, seed, index);
}

// left-to-right fp32 sum, bit-identical to `float s = 0; for (i) s += x[i];` (CMatrix::avg, CMatrix.h:1245-1251), evaluated
// with the parallel parity-transducer scan of kernels_consistency.hip
extern "C" int fav_sequential_sum_f32(const float* x, size_t n, float* sum_out, fav_hipstream_t stream)
{
    FAV_REQUIRE(x && sum_out && n > 0, "fav_sequential_sum_f32: bad argument");
    int rc = ensure_device(); if (rc) return rc;
    return launch_sequential_sum(x, n, sum_out, static_cast<hipStream_t>(stream));
}

// temporal-consistency metric of the reference's -evaluate mode (fast_artistic_video.lua:128-151) without the VGG terms
extern "C" int fav_temporal_loss_host(const float* prev_rgb, const float* cur_rgb, const float* backward_flo, const uint8_t* cert_pgm,
                                      int H, int W, int border_mode, double* loss_host, fav_hipstream_t stream)
{
    FAV_REQUIRE(prev_rgb && cur_rgb && backward_flo && cert_pgm && loss_host && H > 0 && W > 0, "fav_temporal_loss_host: bad argument");
    int rc = ensure_device(); if (rc) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    dev_ptr<double> part;
    rc = dev_alloc(part, 256); if (rc) return rc;
    rc = launch_temporal_loss(prev_rgb, cur_rgb, backward_flo, cert_pgm, border_mode, H, W, part.get(), st);
    double h[256];
    if (!rc && hipMemcpyAsync(h, part.get(), sizeof h, hipMemcpyDeviceToHost, st) != hipSuccess) rc = hip_fail(hipGetLastError(), "hipMemcpyAsync");
    if (!rc && hipStreamSynchronize(st) != hipSuccess) rc = hip_fail(hipGetLastError(), "hipStreamSynchronize");
    if (rc) return rc;
    double s = 0.0;
    for (int i = 0; i < 256; ++i) s += h[i];
    *loss_host = s / (3.0 * (double)H * (double)W);
    return FAV_OK;
}

// ================================================================================================
// host-side formats
// ================================================================================================
extern "C" void fav_free_host(void* p) { free(p); }

// flowFileLoader.lua:14-34 / consistencyChecker.cpp:16-36: float tag (not validated), int32 W, int32 H,
// then H*W interleaved (u, v) little-endian float32
// dst == null: malloc the payload (returned through *uv_out); else read into dst (capacity in floats)
static int read_flo(const char* path, float** uv_out, float* dst, size_t capacity, int* W, int* H)
{
    FILE* f = fopen(path, "rb");
    if (!f) { set_error("Could not open %s", path); return FAV_EIO; }
    float tag; int w = 0, h = 0;
    if (fread(&tag, 4, 1, f) != 1 || fread(&w, 4, 1, f) != 1 || fread(&h, 4, 1, f) != 1 || w <= 0 || h <= 0 ||
        (long long)w * h > (1ll << 28)) {
        fclose(f); set_error("%s: bad .flo header", path); return FAV_EFORMAT; }
    const size_t n = (size_t)w * h * 2;
    if (dst && n > capacity) { fclose(f); set_error("%s: %dx%d flow does not fit the caller's buffer", path, w, h); return FAV_EINVAL; }
    float* d = dst ? dst : static_cast<float*>(malloc(n * sizeof(float)));
    if (!d) { fclose(f); set_error("out of host memory"); return FAV_EIO; }
    if (fread(d, sizeof(float), n, f) != n) { fclose(f); if (!dst) free(d); set_error("%s: truncated .flo payload", path); return FAV_EFORMAT; }
    fclose(f);
    if (uv_out) *uv_out = d;
    *W = w; *H = h;
    return FAV_OK;
}

extern "C" int fav_read_flo_host(const char* path, float** uv_out, int* W, int* H)
{
    FAV_REQUIRE(path && uv_out && W && H, "fav_read_flo_host: null argument");
    return read_flo(path, uv_out, nullptr, 0, W, H);
}

extern "C" int fav_read_flo_into_host(const char* path, float* uv_buf, size_t capacity_floats, int* W, int* H)
{
    FAV_REQUIRE(path && uv_buf && W && H, "fav_read_flo_into_host: null argument");
    return read_flo(path, nullptr, uv_buf, capacity_floats, W, H);
}

static bool pnm_token(FILE* f, char* buf, size_t cap)
{
    int c = fgetc(f);
    for (;;) {
        while (c != EOF && isspace(c)) c = fgetc(f);
        if (c == '#') { while (c != EOF && c != '\n') c = fgetc(f); continue; }
        break;
    }
    size_t n = 0;
    while (c != EOF && !isspace(c) && n + 1 < cap) { buf[n++] = (char)c; c = fgetc(f); }
    buf[n] = 0;
    return n > 0;    // the single whitespace after the token has been consumed
}

// binary P6 / P5, maxval 255 (what ffmpeg and consistencyChecker write; image.load accepts the same)
static int read_pnm(const char* path, uint8_t** data_out, uint8_t* dst, size_t capacity, int* W, int* H, int* channels)
{
    FILE* f = fopen(path, "rb");
    if (!f) { set_error("Could not open %s", path); return FAV_EIO; }
    char tok[64];
    int ch = 0;
    if (pnm_token(f, tok, sizeof tok)) { if (!strcmp(tok, "P6")) ch = 3; else if (!strcmp(tok, "P5")) ch = 1; }
    int w = 0, h = 0, maxv = 0;
    if (ch && pnm_token(f, tok, sizeof tok)) w = atoi(tok);
    if (ch && pnm_token(f, tok, sizeof tok)) h = atoi(tok);
    if (ch && pnm_token(f, tok, sizeof tok)) maxv = atoi(tok);
    if (!ch || w <= 0 || h <= 0 || maxv != 255 || (long long)w * h > (1ll << 28)) {
        fclose(f); set_error("%s: not a binary 8-bit P5/P6 file", path); return FAV_EFORMAT; }
    const size_t n = (size_t)w * h * ch;
    if (dst && n > capacity) { fclose(f); set_error("%s: %dx%dx%d image does not fit the caller's buffer", path, w, h, ch); return FAV_EINVAL; }
    uint8_t* d = dst ? dst : static_cast<uint8_t*>(malloc(n));
    if (!d) { fclose(f); set_error("out of host memory"); return FAV_EIO; }
    if (fread(d, 1, n, f) != n) { fclose(f); if (!dst) free(d); set_error("%s: truncated image payload", path); return FAV_EFORMAT; }
    fclose(f);
    if (data_out) *data_out = d;
    *W = w; *H = h; *channels = ch;
    return FAV_OK;
}

extern "C" int fav_read_pnm_host(const char* path, uint8_t** data_out, int* W, int* H, int* channels)
{
    FAV_REQUIRE(path && data_out && W && H && channels, "fav_read_pnm_host: null argument");
    return read_pnm(path, data_out, nullptr, 0, W, H, channels);
}

extern "C" int fav_read_pnm_into_host(const char* path, uint8_t* buf, size_t capacity_bytes, int* W, int* H, int* channels)
{
    FAV_REQUIRE(path && buf && W && H && channels, "fav_read_pnm_into_host: null argument");
    return read_pnm(path, nullptr, buf, capacity_bytes, W, H, channels);
}

// CMatrix::writeToPGM header (CMatrix.h:1064): "P5\n%d %d\n255\n"; written to a temp file and renamed so
// a polling consumer never sees a partial mask (the reference pre-writes an all-255 file, consistencyChecker.cpp:152)
extern "C" int fav_write_pgm_host(const char* path, const uint8_t* data, int W, int H)
{
    FAV_REQUIRE(path && data && W > 0 && H > 0, "fav_write_pgm_host: bad argument");
    // (the temporary name is per process: two writers of one output -- a caller that gave up on the checker's resident helper next to
    //  the helper itself -- never share a half-written file; whoever renames last wins with complete bytes)
    std::string tmp = std::string(path) + ".tmp." + std::to_string((long long)getpid());
    FILE* f = fopen(tmp.c_str(), "wb");
    if (!f) { set_error("Could not open %s for writing", tmp.c_str()); return FAV_EIO; }
    fprintf(f, "P5\n%d %d\n255\n", W, H);
    const bool ok = fwrite(data, 1, (size_t)W * H, f) == (size_t)W * H;
    if (fclose(f) != 0 || !ok || rename(tmp.c_str(), path) != 0) { unlink(tmp.c_str()); set_error("write to %s failed", path); return FAV_EIO; }
    return FAV_OK;
}

static void put_be32(std::vector<uint8_t>& v, uint32_t x)
{
    v.push_back((uint8_t)(x >> 24)); v.push_back((uint8_t)(x >> 16)); v.push_back((uint8_t)(x >> 8)); v.push_back((uint8_t)x);
}

static void png_chunk(std::vector<uint8_t>& out, const char* type, const uint8_t* data, size_t len)
{
    put_be32(out, (uint32_t)len);
    const size_t start = out.size();
    out.insert(out.end(), type, type + 4);
    if (len) out.insert(out.end(), data, data + len);
    put_be32(out, (uint32_t)crc32(0L, out.data() + start, (uInt)(len + 4)));
}

// image.save("<prefix>-%05d.png") (fast_artistic_video.lua:160-167): 8-bit RGB PNG.  libpng is not
// available in the target image; the container is written directly on top of zlib's deflate.
extern "C" int fav_write_png_rgb8_host(const char* path, const uint8_t* rgb_hwc, int W, int H, int zlib_level)
{
    FAV_REQUIRE(path && rgb_hwc && W > 0 && H > 0, "fav_write_png_rgb8_host: bad argument");
    const size_t stride = (size_t)W * 3;
    // per-thread scratch that persists across calls: a writer pool would otherwise fault in ~8 MB of fresh pages per frame
    // on every thread, and the page-fault path serialises on the process's address-space lock
    static thread_local std::vector<uint8_t> raw, comp, out;
    raw.resize((stride + 1) * H);
    const int level = zlib_level < 0 ? 1 : (zlib_level > 9 ? 9 : zlib_level);
    // Level 0 stores the rows (filter None).  Otherwise every row takes the Sub filter (x - left neighbour, per byte over 3-byte
    // pixels); at the CLI's default level 1 the deflate strategy is Z_RLE: on 1280x720 frames 25 ms per frame and core instead of
    // 85 ms with zlib's default strategy at level 1, and SMALLER files on smooth, textured and noise-like content alike (the
    // filter removes what LZ77 at level 1 would have looked for).  Levels >= 2 keep zlib's default strategy behind the filter.
    for (int y = 0; y < H; ++y) {
        uint8_t* dst = raw.data() + (stride + 1) * y;
        const uint8_t* src = rgb_hwc + stride * y;
        if (level == 0) { dst[0] = 0; memcpy(dst + 1, src, stride); continue; }
        dst[0] = 1;                  // filter type 1 (Sub)
        dst[1] = src[0]; dst[2] = src[1]; dst[3] = src[2];
        for (size_t x = 3; x < stride; ++x) dst[1 + x] = (uint8_t)(src[x] - src[x - 3]);
    }
    uLongf clen = compressBound((uLong)raw.size()) + 64;
    if (comp.size() < clen) comp.resize(clen);
    z_stream zs; memset(&zs, 0, sizeof zs);
    if (deflateInit2(&zs, level, Z_DEFLATED, 15, 8, level == 1 ? Z_RLE : Z_DEFAULT_STRATEGY) != Z_OK) { set_error("zlib deflateInit2 failed"); return FAV_EIO; }
    zs.next_in = raw.data(); zs.avail_in = (uInt)raw.size(); zs.next_out = comp.data(); zs.avail_out = (uInt)clen;
    const int zrc = deflate(&zs, Z_FINISH);
    clen = zs.total_out;
    deflateEnd(&zs);
    if (zrc != Z_STREAM_END) { set_error("zlib deflate failed"); return FAV_EIO; }
    out.clear();
    const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    out.insert(out.end(), sig, sig + 8);
    std::vector<uint8_t> ihdr;
    put_be32(ihdr, (uint32_t)W); put_be32(ihdr, (uint32_t)H);
    ihdr.push_back(8); ihdr.push_back(2); ihdr.push_back(0); ihdr.push_back(0); ihdr.push_back(0);
    png_chunk(out, "IHDR", ihdr.data(), ihdr.size());
    png_chunk(out, "IDAT", comp.data(), clen);
    png_chunk(out, "IEND", nullptr, 0);
    FILE* f = fopen(path, "wb");
    if (!f) { set_error("Could not open %s for writing", path); return FAV_EIO; }
    const bool ok = fwrite(out.data(), 1, out.size(), f) == out.size();
    if (fclose(f) != 0 || !ok) { set_error("write to %s failed", path); return FAV_EIO; }
    return FAV_OK;
}

// ---- YUV4MPEG2 stream header (include/fav.h says which tags are taken); host-only
static bool y4m_int(const char* s, const char* end, int* out)      // [s, end) is a decimal number below 2^30
{
    if (s == end || end - s > 9) return false;
    int v = 0;
    for (; s != end; ++s) { if (*s < '0' || *s > '9') return false; v = v * 10 + (*s - '0'); }
    *out = v;
    return true;
}

static bool y4m_ratio(const std::string& tag, int* num, int* den)   // "<letter><num>:<den>"
{
    const size_t c = tag.find(':');
    return c != std::string::npos && y4m_int(tag.data() + 1, tag.data() + c, num) && y4m_int(tag.data() + c + 1, tag.data() + tag.size(), den);
}

// the C tag of include/fav_yuv.h: "420", "420jpeg", "420mpeg2", "422", "444", "4xxpN"
static bool y4m_colour_space(const std::string& name, fav_yuv_layout* l)
{
    l->depth = 8;
    if (name == "420" || name == "420jpeg") { l->chroma = FAV_YUV_420; l->siting = FAV_YUV_SITING_CENTER; return true; }
    if (name == "420mpeg2") { l->chroma = FAV_YUV_420; l->siting = FAV_YUV_SITING_LEFT; return true; }
    if (name == "444") { l->chroma = FAV_YUV_444; l->siting = FAV_YUV_SITING_CENTER; return true; }
    if (name == "422") { l->chroma = FAV_YUV_422; l->siting = FAV_YUV_SITING_LEFT; return true; }
    if (name.size() < 5 || name[3] != 'p') return false;
    const std::string base = name.substr(0, 3), bits = name.substr(4);
    if (bits != "9" && bits != "10" && bits != "12" && bits != "14" && bits != "16") return false;
    if (base == "420") { l->chroma = FAV_YUV_420; l->siting = FAV_YUV_SITING_CENTER; }
    else if (base == "422") { l->chroma = FAV_YUV_422; l->siting = FAV_YUV_SITING_LEFT; }
    else if (base == "444") { l->chroma = FAV_YUV_444; l->siting = FAV_YUV_SITING_CENTER; }
    else return false;
    l->depth = atoi(bits.c_str());
    return true;
}

// one grammar behind both parsers; every_layout: the C tags of fav_yuv.h, else those of fav.h (h.layout is then 8-bit 4:2:0 / 4:4:4)
static int y4m_parse(const char* line, size_t len, fav_y4m_stream_header* out, bool every_layout);

extern "C" int fav_y4m_parse_header_host(const char* line, size_t len, fav_y4m_header* out)
{
    FAV_REQUIRE(line && out, "fav_y4m_parse_header_host: null argument");
    fav_y4m_stream_header h;
    int rc = y4m_parse(line, len, &h, false); if (rc) return rc;
    memset(out, 0, sizeof *out);
    out->W = h.W; out->H = h.H; out->fps_num = h.fps_num; out->fps_den = h.fps_den; out->aspect_num = h.aspect_num; out->aspect_den = h.aspect_den;
    out->interlace = h.interlace;
    out->fmt = fav_yuv_format{h.layout.chroma, h.layout.siting, h.layout.matrix, h.layout.full_range};
    memcpy(out->xtags, h.xtags, sizeof out->xtags);
    return FAV_OK;
}

extern "C" int fav_y4m_parse_stream_header_host(const char* line, size_t len, fav_y4m_stream_header* out)
{
    FAV_REQUIRE(line && out, "fav_y4m_parse_stream_header_host: null argument");
    return y4m_parse(line, len, out, true);
}

static int y4m_parse(const char* line, size_t len, fav_y4m_stream_header* out, bool every_layout)
{
    size_t n = 0;
    while (n < len && n < FAV_Y4M_MAX_HEADER && line[n] != '\n') ++n;
    FAV_REQUIRE(n < FAV_Y4M_MAX_HEADER, "Y4M header: longer than %d bytes", FAV_Y4M_MAX_HEADER);
    FAV_REQUIRE(n >= 9 && !memcmp(line, "YUV4MPEG2", 9) && (n == 9 || line[9] == ' '), "Y4M header: the stream does not start with YUV4MPEG2");
    fav_y4m_stream_header h;
    memset(&h, 0, sizeof h);
    h.aspect_num = -1;
    h.layout.struct_bytes = sizeof(fav_yuv_layout); h.layout.depth = 8;
    bool have_w = false, have_h = false;
    std::string xt;
    for (size_t p = 9; p < n;) {
        if (line[p] == ' ') { ++p; continue; }
        size_t e = p;
        while (e < n && line[e] != ' ') ++e;
        const std::string tag(line + p, e - p);
        p = e;
        switch (tag[0]) {
        case 'W': FAV_REQUIRE(y4m_int(tag.data() + 1, tag.data() + tag.size(), &h.W) && h.W > 0, "Y4M header: bad tag %s", tag.c_str()); have_w = true; break;
        case 'H': FAV_REQUIRE(y4m_int(tag.data() + 1, tag.data() + tag.size(), &h.H) && h.H > 0, "Y4M header: bad tag %s", tag.c_str()); have_h = true; break;
        case 'F': FAV_REQUIRE(y4m_ratio(tag, &h.fps_num, &h.fps_den) && h.fps_den > 0, "Y4M header: bad tag %s", tag.c_str()); break;
        case 'A': FAV_REQUIRE(y4m_ratio(tag, &h.aspect_num, &h.aspect_den), "Y4M header: bad tag %s", tag.c_str()); break;
        case 'I':
            if (tag == "It" || tag == "Ib" || tag == "Im") { set_error("Y4M header: interlaced material (tag %s) is not supported", tag.c_str()); return FAV_EUNSUPPORTED; }
            FAV_REQUIRE(tag == "Ip" || tag == "I?", "Y4M header: bad tag %s", tag.c_str());
            h.interlace = tag[1];
            break;
        case 'C':
            if (!y4m_colour_space(tag.substr(1), &h.layout) || (!every_layout && (h.layout.depth != 8 || h.layout.chroma == FAV_YUV_422))) {
                if (every_layout) set_error("Y4M header: colour space %s is not supported (C420, C420jpeg, C420mpeg2, C422, C444 and C420pN, C422pN, C444pN with N in 9, 10, 12, 14, 16 are)", tag.c_str());
                else set_error("Y4M header: colour space %s is not supported (8-bit C420, C420jpeg, C420mpeg2 and C444 are)", tag.c_str());
                return FAV_EUNSUPPORTED;
            }
            break;
        case 'X':
            if (tag.compare(0, 12, "XCOLORRANGE=") == 0) {
                FAV_REQUIRE(tag == "XCOLORRANGE=FULL" || tag == "XCOLORRANGE=LIMITED", "Y4M header: bad tag %s", tag.c_str());
                h.layout.full_range = tag == "XCOLORRANGE=FULL";
            }
            xt += (xt.empty() ? "" : " ") + tag;
            break;
        default: FAV_REQUIRE(false, "Y4M header: unknown tag %s", tag.c_str());
        }
    }
    FAV_REQUIRE(have_w && have_h, "Y4M header: the %s tag is missing", have_w ? "H" : "W");
    FAV_REQUIRE((long long)h.W * h.H <= (1ll << 28), "Y4M header: %dx%d frames are too large", h.W, h.H);
    h.layout.matrix = h.H >= 720 ? FAV_YUV_BT709 : FAV_YUV_BT601;      // the stream carries none: the usual player heuristic
    memcpy(h.xtags, xt.c_str(), xt.size() + 1);                     // (shorter than the line, which is shorter than the array)
    *out = h;
    return FAV_OK;
}

// one formatter behind both entry points (`who` names the one called); the layout has been checked
static int y4m_format(const char* who, const fav_y4m_stream_header* h, char* buf_host, size_t capacity);

extern "C" int fav_y4m_format_header_host(const fav_y4m_header* h, char* buf_host, size_t capacity)
{
    FAV_REQUIRE(h && buf_host, "fav_y4m_format_header_host: null argument");
    int rc = yuv_format_check("fav_y4m_format_header_host", h->W, h->H, &h->fmt); if (rc) return rc;
    fav_y4m_stream_header s;
    s.W = h->W; s.H = h->H; s.fps_num = h->fps_num; s.fps_den = h->fps_den; s.aspect_num = h->aspect_num; s.aspect_den = h->aspect_den;
    s.interlace = h->interlace;
    s.layout = fav_yuv_layout{(uint32_t)sizeof(fav_yuv_layout), h->fmt.chroma, h->fmt.chroma == FAV_YUV_444 ? FAV_YUV_SITING_CENTER : h->fmt.siting,
                              h->fmt.matrix, h->fmt.full_range, 8};
    memcpy(s.xtags, h->xtags, sizeof s.xtags);
    return y4m_format("fav_y4m_format_header_host", &s, buf_host, capacity);
}

extern "C" int fav_y4m_format_stream_header_host(const fav_y4m_stream_header* h, char* buf_host, size_t capacity)
{
    FAV_REQUIRE(h && buf_host, "fav_y4m_format_stream_header_host: null argument");
    int rc = yuv_layout_check("fav_y4m_format_stream_header_host", h->W, h->H, &h->layout); if (rc) return rc;
    return y4m_format("fav_y4m_format_stream_header_host", h, buf_host, capacity);
}

static int y4m_format(const char* who, const fav_y4m_stream_header* h, char* buf_host, size_t capacity)
{
    const fav_yuv_layout& l = h->layout;
    const bool left = l.chroma != FAV_YUV_444 && l.siting == FAV_YUV_SITING_LEFT;
    std::string ctag = l.chroma == FAV_YUV_444 ? "C444" : l.chroma == FAV_YUV_422 ? "C422" : l.depth > 8 ? "C420" : left ? "C420mpeg2" : "C420jpeg";
    if (l.depth > 8) ctag += "p" + std::to_string(l.depth);
    if ((l.chroma == FAV_YUV_422 && !left) || (l.chroma == FAV_YUV_420 && left && l.depth > 8)) {
        set_error("%s: YUV4MPEG2 has no colour-space tag for %s: %s is %s-sited", who, l.chroma == FAV_YUV_422 ? "4:2:2 with centre siting" : "left-sited 4:2:0 above 8 bits",
                  ctag.c_str(), l.chroma == FAV_YUV_422 ? "left" : "centre");
        return FAV_EUNSUPPORTED;
    }
    FAV_REQUIRE(h->interlace == 0 || h->interlace == 'p' || h->interlace == '?', "%s: interlace must be 0, 'p' or '?'", who);
    FAV_REQUIRE(memchr(h->xtags, 0, sizeof h->xtags) != nullptr, "%s: xtags is not terminated", who);
    std::string s = "YUV4MPEG2 W" + std::to_string(h->W) + " H" + std::to_string(h->H);
    if (h->fps_den > 0) s += " F" + std::to_string(h->fps_num) + ":" + std::to_string(h->fps_den);
    if (h->interlace) s += std::string(" I") + (char)h->interlace;
    if (h->aspect_num >= 0) s += " A" + std::to_string(h->aspect_num) + ":" + std::to_string(h->aspect_den);
    s += " " + ctag;
    const char* const range = l.full_range ? "XCOLORRANGE=FULL" : "XCOLORRANGE=LIMITED";
    bool range_written = false;
    const std::string xt = h->xtags;
    for (size_t p = 0; p < xt.size();) {
        if (xt[p] == ' ') { ++p; continue; }
        size_t e = xt.find(' ', p);
        if (e == std::string::npos) e = xt.size();
        const std::string tag = xt.substr(p, e - p);
        p = e;
        FAV_REQUIRE(tag[0] == 'X' && tag.find('\n') == std::string::npos, "%s: '%s' in xtags is no X tag", who, tag.c_str());
        if (tag.compare(0, 12, "XCOLORRANGE=") == 0) { if (!range_written) s += std::string(" ") + range; range_written = true; }
        else s += " " + tag;
    }
    if (!range_written && l.full_range) s += std::string(" ") + range;
    s += "\n";
    FAV_REQUIRE(s.size() <= FAV_Y4M_MAX_HEADER, "%s: the header would be longer than %d bytes", who, FAV_Y4M_MAX_HEADER);
    FAV_REQUIRE(s.size() < capacity, "%s: %zu bytes do not fit the caller's buffer", who, s.size() + 1);
    memcpy(buf_host, s.c_str(), s.size() + 1);
    return (int)s.size();
}
