// ops.cpp -- nn.SpatialConvolution / nn.SpatialFullConvolution [+ nn.InstanceNormalization [+ nn.ReLU]] as stand-alone NCHW operators
// (tests / ops): the network's own kernels around a layout conversion on either side.
#include "net_internal.h"
#include "tconv_pack.h"

using namespace fav;

namespace {

// Convolution c (weights, geometry and OH x OW set by the caller; input, bias, output and statistics buffers set here), optional
// InstanceNorm (gamma != null) + ReLU, NCHW out.  in: NCHW [c.cin_real][H][W], laid out as NHWC with c.CIN channels for the kernel;
// tiles / counts: the kernel's partial-statistics tiles, and whether it writes their pixel counts.  Synchronises the stream.
int conv_in_nchw(ConvLaunch c, int (*launch)(const ConvLaunch&, hipStream_t), int tiles, bool counts, const float* in, int H, int W,
                 const float* bias, const float* gamma, const float* beta, float eps, int relu, float* out, hipStream_t st, const char* who)
{
    const int M = c.OH * c.OW;
    std::vector<float> hb((size_t)c.COUTp, 0.f);
    if (bias) FAV_HIP(hipMemcpy(hb.data(), bias, (size_t)c.COUT * sizeof(float), hipMemcpyDeviceToHost));
    dev_ptr<float> db, din, dout, dpart, dss; dev_ptr<int> dcnt;      // dss: scale | shift
    if (dev_upload(db, hb) || dev_alloc(din, (size_t)H * W * c.CIN) || dev_alloc(dout, (size_t)M * c.COUT) ||
        dev_alloc(dpart, (size_t)tiles * c.COUTp * 2) || (counts && dev_alloc(dcnt, (size_t)tiles)) || dev_alloc(dss, (size_t)2 * c.COUTp)) return FAV_EHIP;
    int rc = launch_nchw_to_nhwc_pad(in, c.cin_real, H, W, 0, c.CIN, din.get(), st);
    c.in = din.get(); c.IH = H; c.IW = W; c.IWp = W; c.bias = db.get(); c.out = dout.get();
    c.partials = gamma ? dpart.get() : nullptr; c.counts = dcnt.get();
    if (!rc) rc = launch(c, st);
    Affine t;
    if (!rc && gamma) {
        rc = launch_in_finalize(dpart.get(), c.counts, tiles, M, CONV_BM, c.COUT, c.COUTp, gamma, beta, eps, dss.get(), dss.get() + c.COUTp, st);
        t.scale1 = dss.get(); t.shift1 = dss.get() + c.COUTp; t.relu1 = relu; t.stages = 1;
    }
    if (!rc) rc = launch_nhwc_to_nchw(dout.get(), M, c.COUT, t, out, st);
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
    dev_ptr<float> dw;
    rc = dev_upload(dw, wre); if (rc) return rc;
    c.wgt = dw.get();
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
    dev_ptr<float> dw;
    if (stride == 1) {
        conv_tconv_as_conv(hw.data(), Cin, Cout, k, wpk);
        rc = dev_upload(dw, wpk); if (rc) return rc;
        return fav_conv2d_nchw_f32(in, Cin, H, W, dw.get(), bias, Cout, k, 1, k - 1 - pad, gamma, beta, eps, relu, out, stream);
    }
    ConvLaunch c;
    c.cin_real = Cin; c.CIN = (Cin + 7) / 8 * 8; c.COUT = Cout; c.COUTp = (Cout + 31) / 32 * 32;
    c.KH = c.KW = k; c.stride = stride; c.pad = pad; c.OH = (H - 1) * stride - 2 * pad + k + adj; c.OW = (W - 1) * stride - 2 * pad + k + adj;
    FAV_REQUIRE(c.OH > 0 && c.OW > 0, "fav_conv_transpose2d_nchw_f32: empty output");
    conv_tconv_pack(hw.data(), Cin, Cout, c.CIN, c.COUTp, k, stride, pad, wpk);
    rc = dev_upload(dw, wpk); if (rc) return rc;
    c.wpk = dw.get();
    return conv_in_nchw(c, launch_conv_tconv, conv_tconv_tiles(c), true, in, H, W, bias, gamma, beta, eps, relu, out, static_cast<hipStream_t>(stream), "fav_conv_transpose2d_nchw_f32");
}
