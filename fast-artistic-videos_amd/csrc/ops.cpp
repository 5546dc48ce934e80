// ops.cpp -- nn.SpatialConvolution / nn.SpatialFullConvolution [+ nn.InstanceNormalization [+ nn.ReLU]] as stand-alone NCHW operators
// (tests / ops): the network's own kernels around a layout conversion on either side.
#include "net_internal.h"
#include "tconv_pack.h"

using namespace fav;

namespace {

// a device allocation that frees itself
struct DevMem {
    float* p = nullptr;
    DevMem() = default; DevMem(const DevMem&) = delete; DevMem& operator=(const DevMem&) = delete;
    ~DevMem() { (void)hipFree(p); }
    int alloc(size_t floats) { FAV_HIP(hipMalloc(reinterpret_cast<void**>(&p), (floats ? floats : 1) * sizeof(float))); return FAV_OK; }
    int upload(const std::vector<float>& h, size_t pad_to = 0) { return dev_upload(h, pad_to, &p); }
};

// Convolution c (weights, geometry and OH x OW set by the caller; input, bias, output and statistics buffers set here), optional
// InstanceNorm (gamma != null) + ReLU, NCHW out.  in: NCHW [c.cin_real][H][W], laid out as NHWC with c.CIN channels for the kernel;
// tiles / counts: the kernel's partial-statistics tiles, and whether it writes their pixel counts.  Synchronises the stream.
int conv_in_nchw(ConvLaunch c, int (*launch)(const ConvLaunch&, hipStream_t), int tiles, bool counts, const float* in, int H, int W,
                 const float* bias, const float* gamma, const float* beta, float eps, int relu, float* out, hipStream_t st, const char* who)
{
    const int M = c.OH * c.OW;
    std::vector<float> hb((size_t)c.COUTp, 0.f);
    if (bias) FAV_HIP(hipMemcpy(hb.data(), bias, (size_t)c.COUT * sizeof(float), hipMemcpyDeviceToHost));
    DevMem db, din, dout, dpart, dcnt, dss;      // dss: scale | shift
    int rc = db.upload(hb);
    if (!rc) rc = din.alloc((size_t)H * W * c.CIN);
    if (!rc) rc = dout.alloc((size_t)M * c.COUT);
    if (!rc) rc = dpart.alloc((size_t)tiles * c.COUTp * 2);
    if (!rc && counts) rc = dcnt.alloc((size_t)tiles);
    if (!rc) rc = dss.alloc((size_t)2 * c.COUTp);
    if (rc) return rc;
    rc = launch_nchw_to_nhwc_pad(in, c.cin_real, H, W, 0, c.CIN, din.p, st);
    c.in = din.p; c.IH = H; c.IW = W; c.IWp = W; c.bias = db.p; c.out = dout.p;
    c.partials = gamma ? dpart.p : nullptr; c.counts = reinterpret_cast<int*>(dcnt.p);
    if (!rc) rc = launch(c, st);
    Affine t;
    if (!rc && gamma) {
        rc = launch_in_finalize(dpart.p, c.counts, tiles, M, CONV_BM, c.COUT, c.COUTp, gamma, beta, eps, dss.p, dss.p + c.COUTp, st);
        t.scale1 = dss.p; t.shift1 = dss.p + c.COUTp; t.relu1 = relu; t.stages = 1;
    }
    if (!rc) rc = launch_nhwc_to_nchw(dout.p, M, c.COUT, t, out, st);
    if (hipStreamSynchronize(st) != hipSuccess && !rc) rc = hip_fail(hipGetLastError(), who);
    return rc;
}

}  // namespace

// on the generic kernel (launch_conv), whatever the shape
extern "C" int fav_conv2d_nchw_f32(const float* in, int Cin, int H, int W, const float* weight, const float* bias, int Cout,
                                   int k, int stride, int pad, const float* gamma, const float* beta, float eps, int relu,
                                   float* out, fav_hipstream_t stream)
{
    FAV_REQUIRE(in && weight && out && Cin > 0 && Cout > 0 && k > 0 && stride > 0 && pad >= 0, "fav_conv2d_nchw_f32: bad argument");
    int rc = ensure_device(); if (rc) return rc;
    ConvLaunch c;
    c.cin_real = Cin; c.CIN = (Cin + 3) / 4 * 4; c.COUT = Cout; c.COUTp = (Cout + 31) / 32 * 32; c.Kpad = (k * k * c.CIN + 31) / 32 * 32;
    c.KH = c.KW = k; c.stride = stride; c.pad = pad; c.OH = (H + 2 * pad - k) / stride + 1; c.OW = (W + 2 * pad - k) / stride + 1;
    FAV_REQUIRE(c.OH > 0 && c.OW > 0, "fav_conv2d_nchw_f32: empty output");
    Layer L; L.cin = Cin; L.cout = Cout; L.k = k;
    L.w.resize((size_t)Cin * Cout * k * k);
    FAV_HIP(hipMemcpy(L.w.data(), weight, L.w.size() * sizeof(float), hipMemcpyDeviceToHost));
    std::vector<float> wre;
    repack_weights(L, c.CIN, c.COUTp, c.Kpad, wre);
    DevMem dw;
    rc = dw.upload(wre); if (rc) return rc;
    c.wgt = dw.p;
    return conv_in_nchw(c, launch_conv, conv_tiles(c), false, in, H, W, bias, gamma, beta, eps, relu, out, static_cast<hipStream_t>(stream), "fav_conv2d_nchw_f32");
}

// stride >= 2 on the phase kernel (kernels_tconv.hip), stride 1 as the ordinary convolution it is
extern "C" int fav_conv_transpose2d_nchw_f32(const float* in, int Cin, int H, int W, const float* weight, const float* bias, int Cout,
                                             int k, int stride, int pad, int adj, const float* gamma, const float* beta, float eps, int relu,
                                             float* out, fav_hipstream_t stream)
{
    FAV_REQUIRE(in && weight && out && Cin > 0 && Cout > 0 && H > 0 && W > 0, "fav_conv_transpose2d_nchw_f32: bad argument");
    FAV_REQUIRE(k >= 1 && k <= TCONV_MAX_K && stride >= 1 && stride <= TCONV_MAX_S && pad >= 0 && pad <= k - 1 && adj >= 0 && adj < stride,
                "fav_conv_transpose2d_nchw_f32: supported for k <= %d, stride <= %d, pad <= k - 1, adj < stride, got k=%d s=%d pad=%d adj=%d",
                TCONV_MAX_K, TCONV_MAX_S, k, stride, pad, adj);
    int rc = ensure_device(); if (rc) return rc;
    std::vector<float> hw((size_t)Cin * Cout * k * k), wpk;
    FAV_HIP(hipMemcpy(hw.data(), weight, hw.size() * sizeof(float), hipMemcpyDeviceToHost));
    DevMem dw;
    if (stride == 1) {
        conv_tconv_as_conv(hw.data(), Cin, Cout, k, wpk);
        rc = dw.upload(wpk); if (rc) return rc;
        return fav_conv2d_nchw_f32(in, Cin, H, W, dw.p, bias, Cout, k, 1, k - 1 - pad, gamma, beta, eps, relu, out, stream);
    }
    ConvLaunch c;
    c.cin_real = Cin; c.CIN = (Cin + 7) / 8 * 8; c.COUT = Cout; c.COUTp = (Cout + 31) / 32 * 32;
    c.KH = c.KW = k; c.stride = stride; c.pad = pad; c.OH = (H - 1) * stride - 2 * pad + k + adj; c.OW = (W - 1) * stride - 2 * pad + k + adj;
    FAV_REQUIRE(c.OH > 0 && c.OW > 0, "fav_conv_transpose2d_nchw_f32: empty output");
    conv_tconv_pack(hw.data(), Cin, Cout, c.CIN, c.COUTp, k, stride, pad, wpk);
    rc = dw.upload(wpk); if (rc) return rc;
    c.wpk = dw.p;
    return conv_in_nchw(c, launch_conv_tconv, conv_tconv_tiles(c), true, in, H, W, bias, gamma, beta, eps, relu, out, static_cast<hipStream_t>(stream), "fav_conv_transpose2d_nchw_f32");
}
