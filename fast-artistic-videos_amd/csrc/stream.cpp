// stream.cpp -- host side of the fused per-frame pipeline: look-ahead masks, host-ordered mode, asynchronous PNG encoding, -scale_factor.
//
// fav_stream: replaces one iteration of run_fast_neural_video's loop (core.lua:194-211) with the video
//             CLI's callbacks (fast_artistic_video.lua:93-172), keeping last_frame_stylized on the device.
//
// The network is opaque here: a stream drives its fav_net through the net_* accessors of fav_internal.h (net.cpp), as vr.cpp does.
#include <algorithm>
#include <cstdlib>

#include <unistd.h>

#include "fav_internal.h"

using namespace fav;

// ================================================================================================
// C ABI: fused per-frame pipeline
// ================================================================================================
struct fav_stream {
    fav_net* net = nullptr;
    fav_net* img_net = nullptr;  // optional -model_img: stylises frames that have no prior (core.lua:59-66,146)
    int H = 0, W = 0;            // frame (= flow, certainty, network input) size
    int Ho = 0, Wo = 0;          // network output size: H x W when both are multiples of 4, up to 3 px more otherwise (two stride-2
                                 // convolutions, two x2 upsamplings).  The reference keeps and saves the LARGER image and warps it
                                 // with the flow's size (BilinearSamplerBDHW.lua:71: the output takes the grid's size), so does this
    fav_stream_opts opts{};
    float* state = nullptr;      // last_frame_stylized: [3][Ho][Wo] float RGB, unclamped (fav.lua:169)
    bool has_state = false;
    unsigned frame_counter = 0;  // 1-based index of the frame being stylised (key of the uniform-random fill)
    float* in8 = nullptr;        // padded NHWC8 network input
    // -scale_factor (fav_stream_set_single_image_size): frames without a prior run at sHs x sWs (0: unscaled).  The scaled padded input
    // and the network's planar output at that size (sHo x sWo) live here from the call that sets the size on
    int sHs = 0, sWs = 0, sHo = 0, sWo = 0;
    float* scaled_in8 = nullptr; float* scaled_out = nullptr;
    bool last_scaled = false;    // the last frame ran at the scaled size: in8 does not hold its input
    float* cert_tmp = nullptr; float* cert = nullptr;
    uint8_t* mask = nullptr;     // certainty as the checker writes it (u8 {0,255})
    int* q0_main = nullptr;      // the XCD the caller's queue deals block 0 of a launch to (written by prep_input_kernel, read by the look-ahead mask's long-lived kernels)
    void* ws = nullptr; size_t ws_bytes = 0;
    void* png_ws = nullptr; size_t png_ws_bytes = 0;      // workspace of fav_stream_encode_png (allocated on first use)
    // fav_stream_encode_png_async: the encoder's kernels run on a queue of their own, next to the NEXT frame's network (they fill the
    // tails of its grids instead of standing in front of it).  The state is double-buffered from then on: frame i + 1 is written into
    // the other buffer while frame i's is being encoded, and the frame that comes back to a buffer waits for that buffer's encoder
    hipStream_t png_q = nullptr; hipEvent_t ev_png_in = nullptr;
    float* state_other = nullptr;                         // the buffer `state` is not (null until the first asynchronous encode)
    hipEvent_t png_done = nullptr, png_done_other = nullptr;      // the last encode that read `state` / `state_other` ...
    bool png_pending = false, png_pending_other = false;          // ... if nothing has waited for it yet
    // look-ahead mask (fav_stream_prefetch_mask)
    // two side queues with their own structure workspaces: the masks of frames i+1 and i+2 are computed concurrently
    // (each 4-argument mask contains a ~3 ms sequential fp32 chain, CMatrix::avg), three look-ahead slots
    static constexpr int NSIDE = 2, NPREF = 4;
    hipStream_t side[NSIDE] = {nullptr, nullptr}; void* side_ws[NSIDE] = {nullptr, nullptr}; hipEvent_t ev_in = nullptr;
    float* side_cert_tmp[NSIDE] = {nullptr, nullptr};      // scratch of the certainty preparation (erosion input) on each side queue
    struct Pref { uint8_t* mask = nullptr; float* cert = nullptr; hipEvent_t done = nullptr; bool valid = false;
                  const void *frame = nullptr, *bw = nullptr, *fw = nullptr; int structure = 0;
                  uint32_t retired = 0; };       // host-ordered: retire sequence of the (mask, cert) buffers now in this slot (0: never read)
    Pref pref[NPREF]; int pref_next = 0, side_next = 0;
    // host-ordered look-ahead (fav_stream_set_host_ordered): no event ever enters the caller's queue or the side queues; a one-thread
    // kernel behind the mask pipeline stores a sequence number into host-mapped memory, which fav_stream_next_frame_flow polls
    bool host_ordered = false;
    uint32_t* done_host = nullptr;      // [NPREF], hipHostMalloc
    uint32_t pref_seq[NPREF] = {0, 0, 0, 0}; uint32_t seq_counter = 0;
    // ... and nothing orders a side queue behind the caller's queue either, so the buffers a consumed look-ahead swaps OUT of the stream
    // (read by the previous frames' kernels on the caller's queue) must not be rewritten by a later look-ahead before those kernels are
    // through: the consuming call first enqueues a one-thread kernel on the caller's queue that stores a retire sequence number into
    // host-mapped memory (everything enqueued before it has then finished), and a look-ahead into a slot waits ON THE HOST for the
    // sequence number of the buffers it holds (with NPREF slots and two frames of look-ahead that frame finished long ago: no wait)
    uint32_t* retired_host = nullptr; uint32_t retire_counter = 0;
    hipStream_t last_st = nullptr; bool ran = false;       // the HIP stream of the last forward (forgotten by the destructor)
    ~fav_stream()
    {
        if (net) (void)hipSetDevice(net_device(net));
        if (net && ran) net_forget_stream(net, last_st);
        if (png_q) { (void)hipStreamSynchronize(png_q); (void)hipStreamDestroy(png_q); }
        if (ev_png_in) (void)hipEventDestroy(ev_png_in);
        if (png_done) (void)hipEventDestroy(png_done);
        if (png_done_other) (void)hipEventDestroy(png_done_other);
        (void)hipFree(state_other);
        for (int i = 0; i < NSIDE; ++i) { if (side[i]) { (void)hipStreamSynchronize(side[i]); (void)hipStreamDestroy(side[i]); } (void)hipFree(side_ws[i]); }
        if (ev_in) (void)hipEventDestroy(ev_in);
        if (done_host) (void)hipHostFree(done_host);       // (retired_host lives in the same allocation)
        for (auto& pf : pref) { if (pf.done) (void)hipEventDestroy(pf.done); (void)hipFree(pf.mask); (void)hipFree(pf.cert); }
        for (int i = 0; i < NSIDE; ++i) (void)hipFree(side_cert_tmp[i]);
        (void)hipFree(scaled_in8); (void)hipFree(scaled_out);
        (void)hipFree(q0_main); (void)hipFree(state); (void)hipFree(in8); (void)hipFree(cert_tmp); (void)hipFree(cert); (void)hipFree(mask); (void)hipFree(ws); (void)hipFree(png_ws);
    }
};

// While look-ahead masks are in flight the persistent / stream-K convolution grids leave SIDE_CUS CUs unclaimed
// (fav_net::reserve_cus): the side queues' kernels (among them a ~3 ms single-wave sequential chain) find free CUs, and a
// statically scheduled network block is never kept off the chip by them.
static const int SIDE_CUS = getenv("FAV_SIDE_CUS") ? std::max(0, atoi(getenv("FAV_SIDE_CUS"))) : 4;      // (tuning: read once; 8 until round 4, when a
                                                                                                          //  mask was 1.5 ms of mostly sequential kernels: profiles/r4b_4arg_*)
// one side queue carries every look-ahead since round 4 (a mask is 0.6 ms of short kernels, two in flight fit a 1.8 ms frame back to
// back; two queues measured 541-543 frames/s against 546-548: profiles/r04c_4arg_knobs_ab.log)
static const int NSIDE_USED = getenv("FAV_SIDE_QUEUES") ? std::max(1, std::min(2, atoi(getenv("FAV_SIDE_QUEUES")))) : 1;
// the look-ahead mask's long-lived kernels (the recursive-filter passes) are packed onto the reserved CUs (launch_structure's pack_cus;
// FAV_SIDE_PACK=0: one block per wave, the form of rounds 4-5)
static const int SIDE_PACK = diag_env("FAV_SIDE_PACK") ? std::max(0, atoi(diag_env("FAV_SIDE_PACK"))) : -1;
static hipError_t create_side_stream(hipStream_t* st)
{
    // (confining the side queues with a CU mask -- hipExtStreamCreateWithCUMask -- measured slower than leaving the CUs free, rounds 2-3)
    // FAV_SIDE_CU_MASK=<comma-separated bit numbers>: experiment, round 6
    if (const char* m = diag_env("FAV_SIDE_CU_MASK")) {
        uint32_t words[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (const char* p = m; *p;) { const int b = atoi(p); if (b >= 0 && b < 256) words[b / 32] |= 1u << (b % 32); while (*p && *p != ',') ++p; if (*p == ',') ++p; }
        return hipExtStreamCreateWithCUMask(st, 8, words);
    }
    return hipStreamCreateWithFlags(st, hipStreamNonBlocking);
}

extern "C" int fav_stream_create(fav_net* net, int H, int W, const fav_stream_opts* o, fav_stream** out)
{
    FAV_REQUIRE(net && out && H > 0 && W > 0, "fav_stream_create: bad argument");
    const int pad = net_pad(net);
    FAV_REQUIRE(pad < H && pad < W, "fav_stream_create: %dx%d is smaller than the reflection padding %d", W, H, pad);
    int Ho, Wo; net_out_size(net, H, W, &Ho, &Wo);
    FAV_REQUIRE(Ho >= 1 && Wo >= 1, "frame size %dx%d is too small for the architecture", W, H);
    FAV_HIP(hipSetDevice(net_device(net)));
    fav_stream* s = new fav_stream();
    s->net = net; s->H = H; s->W = W; s->Ho = Ho; s->Wo = Wo;
    if (o) s->opts = *o; else { s->opts.border_mode = FAV_BORDER_STN; s->opts.occlusions_min_filter = 7; s->opts.invert_occlusion = 0; s->opts.fix_occlusions = 0; s->opts.fill_random = 0; s->opts.seed = 0; }
    if (s->opts.occlusions_min_filter < 1) s->opts.occlusions_min_filter = 1;
    const size_t n = (size_t)H * W;
    s->ws_bytes = structure_workspace_bytes(W, H);
    if (hipMalloc(reinterpret_cast<void**>(&s->state), (size_t)3 * Ho * Wo * 4) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&s->in8), (size_t)(H + 2 * pad) * (W + 2 * pad) * 32) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&s->cert_tmp), n * 4) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&s->cert), n * 4) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&s->mask), n) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&s->q0_main), 64) != hipSuccess || hipMemset(s->q0_main, 0, 64) != hipSuccess ||
        hipEventCreateWithFlags(&s->ev_in, hipEventDisableTiming | hipEventDisableSystemFence) != hipSuccess ||
        hipMalloc(&s->ws, s->ws_bytes) != hipSuccess) { delete s; return hip_fail(hipErrorOutOfMemory, "hipMalloc(stream buffers)"); }
    for (auto& pf : s->pref)
        if (hipMalloc(reinterpret_cast<void**>(&pf.mask), n) != hipSuccess || hipMalloc(reinterpret_cast<void**>(&pf.cert), n * 4) != hipSuccess || hipEventCreateWithFlags(&pf.done, hipEventDisableTiming | hipEventDisableSystemFence) != hipSuccess) {
            delete s; return hip_fail(hipErrorOutOfMemory, "look-ahead slots"); }
    for (int i = 0; i < fav_stream::NSIDE; ++i)
        if (create_side_stream(&s->side[i]) != hipSuccess || hipMalloc(&s->side_ws[i], s->ws_bytes) != hipSuccess ||
            hipMalloc(reinterpret_cast<void**>(&s->side_cert_tmp[i]), n * 4) != hipSuccess) {
            delete s; return hip_fail(hipErrorOutOfMemory, "side queues"); }
    *out = s;
    return FAV_OK;
}

extern "C" void fav_stream_destroy(fav_stream* s) { delete s; }

// `state` and `state_other` trade places, each with the event and the flag of the last encode that read it
static void swap_state_buffers(fav_stream* s)
{
    std::swap(s->state, s->state_other);
    std::swap(s->png_done, s->png_done_other);
    std::swap(s->png_pending, s->png_pending_other);
}

// the buffer the next frame is written into becomes `state`.  Synchronous encodes only: the one buffer, in place (the frame's own
// input was assembled from it before the network starts).  With an asynchronous encode possibly reading `state`: the other buffer,
// behind the encode that read THAT one two frames ago (long finished)
static int state_for_writing(fav_stream* s, hipStream_t st)
{
    if (!s->state_other) return FAV_OK;
    swap_state_buffers(s);
    if (s->png_pending) { FAV_HIP(hipStreamWaitEvent(st, s->png_done, 0)); s->png_pending = false; }
    return FAV_OK;
}

// the forward that was to fill the buffer state_for_writing() switched to has failed: `state` names the last COMPLETE frame again
static void state_writing_failed(fav_stream* s)
{
    if (!s->state_other) return;
    swap_state_buffers(s);
}

static int stream_finish(fav_stream* s, float* out_rgb_f32, uint8_t* out_rgb8_hwc, hipStream_t st)
{
    const size_t n = (size_t)s->Ho * s->Wo;
    s->has_state = true;
    if (out_rgb_f32) FAV_HIP(hipMemcpyAsync(out_rgb_f32, s->state, 3 * n * 4, hipMemcpyDeviceToDevice, st));
    if (out_rgb8_hwc) return launch_quantize_rgb8(s->state, out_rgb8_hwc, s->Ho, s->Wo, st);
    return FAV_OK;
}

extern "C" int fav_stream_first_frame(fav_stream* s, const uint8_t* frame_rgb_hwc, float* out_rgb_f32, uint8_t* out_rgb8_hwc,
                                      fav_hipstream_t stream)
{
    FAV_REQUIRE(s && frame_rgb_hwc, "fav_stream_first_frame: null argument");
    FAV_HIP(hipSetDevice(net_device(s->net)));
    hipStream_t st = static_cast<hipStream_t>(stream);
    ++s->frame_counter;
    fav_net* fn = s->img_net ? s->img_net : s->net;      // image model: 3 content channels (the zero prior / mask planes meet zero weights)
    if (s->sHs) {      // core.lua:127-130,150-152: resampled before the model, the result resampled back to H x W (= Ho x Wo) into the state
        int rc = launch_scale_prep(frame_rgb_hwc, s->H, s->W, s->sHs, s->sWs, net_pad(s->net), s->scaled_in8, st,
                                   s->img_net ? 0 : s->opts.fill_random, s->opts.seed, s->frame_counter);
        if (rc) return rc;
        s->last_st = st; s->ran = true; s->last_scaled = true;
        rc = state_for_writing(s, st); if (rc) return rc;
        rc = net_forward_padded(fn, s->scaled_in8, s->sHs, s->sWs, s->scaled_out, st);
        if (!rc) rc = launch_scale_planar(s->scaled_out, s->state, 3, s->sHo, s->sWo, s->Ho, s->Wo, st);
        if (rc) { state_writing_failed(s); return rc; }
        return stream_finish(s, out_rgb_f32, out_rgb8_hwc, st);
    }
    // the image model sees only the three content channels (core.lua:146): no fill there
    int rc = launch_prep_input(frame_rgb_hwc, nullptr, 0, 0, nullptr, nullptr, s->opts.border_mode, s->H, s->W, net_pad(s->net), s->in8, st,
                               s->img_net ? 0 : s->opts.fill_random, s->opts.seed, s->frame_counter);
    if (rc) return rc;
    s->last_st = st; s->ran = true; s->last_scaled = false;
    rc = state_for_writing(s, st); if (rc) return rc;
    rc = net_forward_padded(fn, s->in8, s->H, s->W, s->state, st); if (rc) { state_writing_failed(s); return rc; }
    return stream_finish(s, out_rgb_f32, out_rgb8_hwc, st);
}

extern "C" int fav_stream_set_image_net(fav_stream* s, fav_net* image_net)
{
    FAV_REQUIRE(s, "fav_stream_set_image_net: null stream");
    if (image_net) {
        FAV_REQUIRE(net_device(image_net) == net_device(s->net), "fav_stream_set_image_net: the image model lives on another device");
        FAV_REQUIRE(net_pad(image_net) == net_pad(s->net), "fav_stream_set_image_net: image model pads %d px, video model %d px (both read the same padded input)", net_pad(image_net), net_pad(s->net));
        int Ho, Wo; net_out_size(image_net, s->H, s->W, &Ho, &Wo);
        FAV_REQUIRE(Ho == s->Ho && Wo == s->Wo, "fav_stream_set_image_net: the image model maps %dx%d to %dx%d, the video model to %dx%d", s->W, s->H, Wo, Ho, s->Wo, s->Ho);
        if (s->sHs) {
            net_out_size(image_net, s->sHs, s->sWs, &Ho, &Wo);
            FAV_REQUIRE(Ho == s->sHo && Wo == s->sWo, "fav_stream_set_image_net: the image model maps the scaled %dx%d to %dx%d, the video model to %dx%d", s->sWs, s->sHs, Wo, Ho, s->sWo, s->sHo);
        }
    }
    s->img_net = image_net;
    return FAV_OK;
}

extern "C" int fav_stream_set_single_image_size(fav_stream* s, int Hs, int Ws)
{
    FAV_REQUIRE(s, "fav_stream_set_single_image_size: null stream");
    FAV_HIP(hipSetDevice(net_device(s->net)));
    if (Hs == 0 && Ws == 0) {      // back to the unscaled path (hipFree waits for the frames that still read the buffers)
        (void)hipFree(s->scaled_in8); (void)hipFree(s->scaled_out);
        s->scaled_in8 = s->scaled_out = nullptr; s->sHs = s->sWs = s->sHo = s->sWo = 0;
        return FAV_OK;
    }
    if (s->Ho != s->H || s->Wo != s->W) {
        set_error("fav_stream_set_single_image_size: the network maps %dx%d frames to %dx%d; the result is scaled back to the frame's size (core.lua:151), "
                  "which must therefore be the size of the stylised frames (both sides multiples of 4 for the canonical models)", s->W, s->H, s->Wo, s->Ho);
        return FAV_EUNSUPPORTED;
    }
    const int pad = net_pad(s->net);
    FAV_REQUIRE(Hs > 0 && Ws > 0 && pad < Hs && pad < Ws, "fav_stream_set_single_image_size: %dx%d is not larger than the reflection padding %d", Ws, Hs, pad);
    int Ho, Wo; net_out_size(s->net, Hs, Ws, &Ho, &Wo);
    FAV_REQUIRE(Ho >= 1 && Wo >= 1, "fav_stream_set_single_image_size: %dx%d is too small for the architecture", Ws, Hs);
    if (s->img_net) {
        int Hi, Wi; net_out_size(s->img_net, Hs, Ws, &Hi, &Wi);
        FAV_REQUIRE(Hi == Ho && Wi == Wo, "fav_stream_set_single_image_size: the image model maps %dx%d to %dx%d, the video model to %dx%d", Ws, Hs, Wi, Hi, Wo, Ho);
    }
    float* in8 = nullptr; float* out = nullptr;
    if (hipMalloc(reinterpret_cast<void**>(&in8), (size_t)(Hs + 2 * pad) * (Ws + 2 * pad) * 32) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&out), (size_t)3 * Ho * Wo * 4) != hipSuccess) {
        (void)hipFree(in8); return hip_fail(hipErrorOutOfMemory, "hipMalloc(scaled single-image buffers)"); }
    (void)hipFree(s->scaled_in8); (void)hipFree(s->scaled_out);
    s->scaled_in8 = in8; s->scaled_out = out; s->sHs = Hs; s->sWs = Ws; s->sHo = Ho; s->sWo = Wo;
    return FAV_OK;
}

// cert_ready: the certainty (mask options + erosion applied) is already in s->cert (computed ahead on a side queue)
// input_ready: ... and the network input in s->in8 as well (fav_stream_next_frame_flow's fused check + assembly; frame_counter advanced)
static int stream_next(fav_stream* s, const uint8_t* frame, const float* bw, const uint8_t* mask, float* out_f32, uint8_t* out_u8,
                       hipStream_t st, bool cert_ready = false, bool input_ready = false)
{
    FAV_REQUIRE(s->has_state, "fav_stream_next_frame: no previous stylised frame (call fav_stream_first_frame or fav_stream_set_state first)");
    int rc = FAV_OK;
    if (!input_ready) {
        TraceRange tr_pre("fav:certainty+warp+assemble");
        if (!cert_ready)
            rc = launch_cert_prepare(mask, bw, s->opts.invert_occlusion, s->opts.fix_occlusions, s->opts.border_mode,
                                     s->opts.occlusions_min_filter, s->cert_tmp, s->cert, s->H, s->W, st);
        if (rc) return rc;
        ++s->frame_counter;
        rc = launch_prep_input(frame, s->state, s->Ho, s->Wo, bw, s->cert, s->opts.border_mode, s->H, s->W, net_pad(s->net), s->in8, st,
                               s->opts.fill_random, s->opts.seed, s->frame_counter, s->q0_main);
        if (rc) return rc;
    }
    s->last_st = st; s->ran = true; s->last_scaled = false;
    rc = state_for_writing(s, st); if (rc) return rc;       // (the prior was read from the previous state above)
    { TraceRange tr_net("fav:network"); rc = net_forward_padded(s->net, s->in8, s->H, s->W, s->state, st); }
    if (rc) { state_writing_failed(s); return rc; }
    return stream_finish(s, out_f32, out_u8, st);
}

extern "C" int fav_stream_next_frame_cert(fav_stream* s, const uint8_t* frame_rgb_hwc, const float* backward_flo,
                                          const uint8_t* cert_pgm, float* out_rgb_f32, uint8_t* out_rgb8_hwc,
                                          fav_hipstream_t stream)
{
    FAV_REQUIRE(s && frame_rgb_hwc && backward_flo && cert_pgm, "fav_stream_next_frame_cert: null argument");
    FAV_HIP(hipSetDevice(net_device(s->net)));
    hipStream_t st = static_cast<hipStream_t>(stream);
    FAV_HIP(hipMemcpyAsync(s->mask, cert_pgm, (size_t)s->H * s->W, hipMemcpyDeviceToDevice, st));
    return stream_next(s, frame_rgb_hwc, backward_flo, s->mask, out_rgb_f32, out_rgb8_hwc, st);
}

extern "C" int fav_stream_next_frame_flow(fav_stream* s, const uint8_t* frame_rgb_hwc, const float* backward_flo,
                                          const float* forward_flo, int use_structure, float* out_rgb_f32,
                                          uint8_t* out_rgb8_hwc, fav_hipstream_t stream)
{
    FAV_REQUIRE(s && frame_rgb_hwc && backward_flo && forward_flo, "fav_stream_next_frame_flow: null argument");
    FAV_HIP(hipSetDevice(net_device(s->net)));
    hipStream_t st = static_cast<hipStream_t>(stream);
    // makeOptFlow_deepflow.sh:59: consistencyChecker backward_i_j.flo forward_j_i.flo reliable_i_j.pgm [frame_i.ppm]
    for (auto& pf : s->pref)
        if (pf.valid && pf.frame == frame_rgb_hwc && pf.bw == backward_flo && pf.fw == forward_flo && pf.structure == (use_structure != 0)) {
            // the mask was computed ahead of time on the side stream
            pf.valid = false;
            if (s->host_ordered) {
                // the mask pipeline of this slot ends in a store of its sequence number to host-mapped memory: wait for it HERE, on the
                // host (it was started a frame ago: normally no wait at all), then enqueue -- no dependency between the queues
                const int slot = (int)(&pf - s->pref);
                volatile uint32_t* flag = &s->done_host[slot];
                for (int spins = 0; *flag != s->pref_seq[slot]; ++spins) {
                    usleep(50);
                    if ((spins & 2047) == 2047) { const hipError_t e = hipStreamQuery(s->side[0]); if (e != hipSuccess && e != hipErrorNotReady) return hip_fail(e, "look-ahead queue"); }
                }
                // the buffers about to leave the stream were read by kernels already in the caller's queue: mark the point behind them
                pf.retired = ++s->retire_counter;
                int rcf = launch_store_flag(s->retired_host, pf.retired, st); if (rcf) return rcf;
            } else FAV_HIP(hipStreamWaitEvent(st, pf.done, 0));
            std::swap(s->mask, pf.mask);
            std::swap(s->cert, pf.cert);          // mask -> certainty (options, erosion) was done on the side queue as well
            return stream_next(s, frame_rgb_hwc, backward_flo, s->mask, out_rgb_f32, out_rgb8_hwc, st, true);
        }
    // not prefetched: compute inline on the caller's stream (own workspace)
    TraceRange tr_mask("fav:consistency mask");
    const float* structure = nullptr; const float* avg = nullptr;
    if (use_structure) {
        int rc = launch_structure(frame_rgb_hwc, s->W, s->H, s->ws, s->ws_bytes, &structure, &avg, st); if (rc) return rc;
    }
    // check + certainty options + erosion + input assembly in ONE tile kernel (round 5; the mask byte and the eroded certainty of every pixel
    // are still written: fav_stream_last_mask); FAV_NO_CHECK_PREP: the check and the assembly as two launches (rounds 3-4)
    static const bool fused_prep = diag_env("FAV_NO_CHECK_PREP") == nullptr;      // (tuning: read once)
    if (fused_prep && s->has_state) {
        ++s->frame_counter;
        int rcp = launch_check_prep(frame_rgb_hwc, s->state, s->Ho, s->Wo, backward_flo, forward_flo, structure, avg, s->mask, s->cert,
                                    s->opts.invert_occlusion, s->opts.fix_occlusions, s->opts.border_mode, s->opts.occlusions_min_filter,
                                    s->H, s->W, net_pad(s->net), s->in8, st, s->opts.fill_random, s->opts.seed, s->frame_counter);
        if (rcp) return rcp;
        return stream_next(s, frame_rgb_hwc, backward_flo, s->mask, out_rgb_f32, out_rgb8_hwc, st, true, true);
    }
    int rc = launch_check_cert(backward_flo, forward_flo, structure, avg, s->mask, s->opts.invert_occlusion, s->opts.fix_occlusions, s->opts.border_mode,
                               s->opts.occlusions_min_filter, s->cert, s->H, s->W, st);
    if (rc) return rc;
    return stream_next(s, frame_rgb_hwc, backward_flo, s->mask, out_rgb_f32, out_rgb8_hwc, st, true);
}

// -estimate_flow: both flows from the two frames on the caller's queue, then the frame as above (never prefetched: the flows do not exist
// before this call).  A workspace of fav_flow_pairs_workspace_bytes(W, H, 1) bytes gets the batch of one: each frame's pyramid built once,
// both flows in every launch, the same bits.  The smaller fav_flow_workspace_bytes that callers have always passed holds one flow at a
// time: two single calls
extern "C" int fav_stream_next_frame_estimate(fav_stream* s, const uint8_t* frame_rgb_hwc, const uint8_t* prev_frame_rgb_hwc,
                                              const fav_flow_opts* flow_opts_host, int use_structure, float* backward_flo, float* forward_flo,
                                              void* workspace, size_t workspace_bytes, float* out_rgb_f32, uint8_t* out_rgb8_hwc,
                                              fav_hipstream_t stream)
{
    const fav_flow_opts_ex ex = flow_opts_brightness(flow_opts_host);
    return fav_stream_next_frame_estimate_ex(s, frame_rgb_hwc, prev_frame_rgb_hwc, &ex, use_structure, backward_flo, forward_flo, workspace, workspace_bytes,
                                             out_rgb_f32, out_rgb8_hwc, stream);
}

extern "C" int fav_stream_next_frame_estimate_ex(fav_stream* s, const uint8_t* frame_rgb_hwc, const uint8_t* prev_frame_rgb_hwc,
                                                 const fav_flow_opts_ex* flow_opts_host, int use_structure, float* backward_flo, float* forward_flo,
                                                 void* workspace, size_t workspace_bytes, float* out_rgb_f32, uint8_t* out_rgb8_hwc,
                                                 fav_hipstream_t stream)
{
    const fav_flow_opts_ex2 ex2 = flow_opts_no_match(flow_opts_host);
    return fav_stream_next_frame_estimate_ex2(s, frame_rgb_hwc, prev_frame_rgb_hwc, &ex2, use_structure, backward_flo, forward_flo, workspace, workspace_bytes,
                                              out_rgb_f32, out_rgb8_hwc, stream);
}

extern "C" int fav_stream_next_frame_estimate_ex2(fav_stream* s, const uint8_t* frame_rgb_hwc, const uint8_t* prev_frame_rgb_hwc,
                                                  const fav_flow_opts_ex2* flow_opts_host, int use_structure, float* backward_flo, float* forward_flo,
                                                  void* workspace, size_t workspace_bytes, float* out_rgb_f32, uint8_t* out_rgb8_hwc,
                                                  fav_hipstream_t stream)
{
    FAV_REQUIRE(s && frame_rgb_hwc && prev_frame_rgb_hwc && backward_flo && forward_flo, "fav_stream_next_frame_estimate: null argument");
    FAV_HIP(hipSetDevice(net_device(s->net)));
    const size_t pair_bytes = fav_flow_pairs_workspace_bytes_ex2(s->W, s->H, 1, flow_opts_host);      // (0: a bad option; the single call reports it)
    int rc;
    if (pair_bytes && workspace_bytes >= pair_bytes) {
        rc = fav_flow_pairs_rgb8_ex2(&prev_frame_rgb_hwc, &frame_rgb_hwc, 1, s->W, s->H, flow_opts_host, &backward_flo, &forward_flo, workspace,
                                     workspace_bytes, stream);
        if (rc) return rc;
    } else {
        rc = fav_flow_rgb8_ex2(frame_rgb_hwc, prev_frame_rgb_hwc, s->W, s->H, flow_opts_host, backward_flo, workspace, workspace_bytes, stream);
        if (rc) return rc;
        rc = fav_flow_rgb8_ex2(prev_frame_rgb_hwc, frame_rgb_hwc, s->W, s->H, flow_opts_host, forward_flo, workspace, workspace_bytes, stream);
        if (rc) return rc;
    }
    return fav_stream_next_frame_flow(s, frame_rgb_hwc, backward_flo, forward_flo, use_structure, out_rgb_f32, out_rgb8_hwc, stream);
}

extern "C" int fav_stream_prefetch_mask(fav_stream* s, const uint8_t* frame_rgb_hwc, const float* backward_flo,
                                        const float* forward_flo, int use_structure, fav_hipstream_t stream)
{
    FAV_REQUIRE(s && frame_rgb_hwc && backward_flo && forward_flo, "fav_stream_prefetch_mask: null argument");
    FAV_HIP(hipSetDevice(net_device(s->net)));
    hipStream_t st = static_cast<hipStream_t>(stream);
    // the 4-argument mask holds long sequential chains: from now on the network's persistent grids leave the side queues their CUs;
    // the 3-argument mask + certainty (25 us of small kernels) fits into the grids' own tails
    if (use_structure) net_reserve_cus(s->net, SIDE_CUS);
    fav_stream::Pref& pf = s->pref[s->pref_next];
    s->pref_next = (s->pref_next + 1) % fav_stream::NPREF;
    const int q = s->side_next; s->side_next = (s->side_next + 1) % NSIDE_USED;
    hipStream_t sd = s->side[q];
    if (!s->host_ordered) {
        FAV_HIP(hipEventRecord(s->ev_in, st));                 // inputs are complete at this point of the caller's stream
        FAV_HIP(hipStreamWaitEvent(sd, s->ev_in, 0));          // (work enqueued on `stream` AFTER this call is not waited for)
    } else if (pf.retired) {                                   // host-ordered: the caller has SEEN the inputs complete (fav.h) ...
        // ... and the slot's buffers were read by frames on the caller's queue: those must be through before a side queue rewrites them
        volatile uint32_t* flag = s->retired_host;
        for (int spins = 0; (int32_t)(*flag - pf.retired) < 0; ++spins) {
            usleep(50);
            if ((spins & 2047) == 2047) { const hipError_t e = hipStreamQuery(st); if (e != hipSuccess && e != hipErrorNotReady) return hip_fail(e, "look-ahead: the caller's queue"); }
        }
        pf.retired = 0;
    }
    const float* structure = nullptr; const float* avg = nullptr;
    if (use_structure) {
        int rc = launch_structure(frame_rgb_hwc, s->W, s->H, s->side_ws[q], s->ws_bytes, &structure, &avg, sd, SIDE_PACK >= 0 ? SIDE_PACK : SIDE_CUS, s->q0_main); if (rc) return rc;
    }
    // mask + certainty of the frame (mask options, fix_occlusions warp of ones, erosion): depends on the flows and the stream's options only
    int rc = launch_check_cert(backward_flo, forward_flo, structure, avg, pf.mask, s->opts.invert_occlusion, s->opts.fix_occlusions, s->opts.border_mode,
                               s->opts.occlusions_min_filter, pf.cert, s->H, s->W, sd);
    if (rc) return rc;
    if (s->host_ordered) {
        const int slot = (int)(&pf - s->pref);
        s->pref_seq[slot] = ++s->seq_counter;
        rc = launch_store_flag(&s->done_host[slot], s->pref_seq[slot], sd); if (rc) return rc;
    } else FAV_HIP(hipEventRecord(pf.done, sd));
    pf.valid = true; pf.frame = frame_rgb_hwc; pf.bw = backward_flo; pf.fw = forward_flo; pf.structure = use_structure != 0;
    return FAV_OK;
}

extern "C" int fav_stream_get_state(fav_stream* s, float* state_rgb_f32, fav_hipstream_t stream)
{
    FAV_REQUIRE(s && state_rgb_f32 && s->has_state, "fav_stream_get_state: no state");
    FAV_HIP(hipSetDevice(net_device(s->net)));
    FAV_HIP(hipMemcpyAsync(state_rgb_f32, s->state, (size_t)3 * s->Ho * s->Wo * 4, hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)));
    return FAV_OK;
}

extern "C" int fav_stream_set_state(fav_stream* s, const float* state_rgb_f32, fav_hipstream_t stream)
{
    FAV_REQUIRE(s && state_rgb_f32, "fav_stream_set_state: null argument");
    FAV_HIP(hipSetDevice(net_device(s->net)));
    if (s->png_pending) { FAV_HIP(hipStreamWaitEvent(static_cast<hipStream_t>(stream), s->png_done, 0)); s->png_pending = false; }
    FAV_HIP(hipMemcpyAsync(s->state, state_rgb_f32, (size_t)3 * s->Ho * s->Wo * 4, hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)));
    s->has_state = true;
    return FAV_OK;
}

extern "C" int fav_stream_wait_png(fav_stream* s, fav_hipstream_t stream)
{
    FAV_REQUIRE(s, "fav_stream_wait_png: null stream");
    FAV_HIP(hipSetDevice(net_device(s->net)));
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (s->png_pending) FAV_HIP(hipStreamWaitEvent(st, s->png_done, 0));
    if (s->png_pending_other) FAV_HIP(hipStreamWaitEvent(st, s->png_done_other, 0));
    return FAV_OK;
}

// the encoder's workspace, allocated on first use (both encode calls share the one)
static int ensure_png_ws(fav_stream* s)
{
    if (s->png_ws) return FAV_OK;
    s->png_ws_bytes = png_workspace_bytes(s->Wo, s->Ho);
    FAV_HIP(hipMalloc(&s->png_ws, s->png_ws_bytes));
    return FAV_OK;
}

extern "C" int fav_stream_encode_png(fav_stream* s, void* png_out, size_t capacity, uint32_t* png_bytes_out, fav_hipstream_t stream)
{
    FAV_REQUIRE(s && s->has_state, "fav_stream_encode_png: no stylised frame yet");
    FAV_HIP(hipSetDevice(net_device(s->net)));
    { int rc = ensure_png_ws(s); if (rc) return rc; }
    if (s->png_q) { int rc = fav_stream_wait_png(s, stream); if (rc) return rc; }      // (one workspace: behind the asynchronous encodes)
    return launch_png_encode(nullptr, s->state, s->Wo, s->Ho, png_out, capacity, png_bytes_out, s->png_ws, s->png_ws_bytes, static_cast<hipStream_t>(stream));
}

extern "C" int fav_stream_encode_png_async(fav_stream* s, void* png_out, size_t capacity, uint32_t* png_bytes_out, fav_hipstream_t stream)
{
    FAV_REQUIRE(s && s->has_state, "fav_stream_encode_png_async: no stylised frame yet");
    FAV_HIP(hipSetDevice(net_device(s->net)));
    hipStream_t st = static_cast<hipStream_t>(stream);
    { int rc = ensure_png_ws(s); if (rc) return rc; }
    if (!s->png_q) {
        // all or nothing: a stream with the queue but without the second state buffer would let the next frame overwrite what is being encoded
        const unsigned ef = hipEventDisableTiming | hipEventDisableSystemFence;
        hipStream_t q = nullptr; hipEvent_t e0 = nullptr, e1 = nullptr, e2 = nullptr; float* other = nullptr;
        const hipError_t e = [&]() -> hipError_t {
            hipError_t r;
            if ((r = hipStreamCreateWithFlags(&q, hipStreamNonBlocking)) != hipSuccess) return r;
            if ((r = hipEventCreateWithFlags(&e0, ef)) != hipSuccess) return r;
            if ((r = hipEventCreateWithFlags(&e1, ef)) != hipSuccess) return r;
            if ((r = hipEventCreateWithFlags(&e2, ef)) != hipSuccess) return r;
            return hipMalloc(reinterpret_cast<void**>(&other), (size_t)3 * s->Ho * s->Wo * 4);
        }();
        if (e != hipSuccess) {
            if (q) (void)hipStreamDestroy(q);
            if (e0) (void)hipEventDestroy(e0);
            if (e1) (void)hipEventDestroy(e1);
            if (e2) (void)hipEventDestroy(e2);
            (void)hipFree(other);
            return hip_fail(e, "fav_stream_encode_png_async: encoder queue / second state buffer");
        }
        s->png_q = q; s->ev_png_in = e0; s->png_done = e1; s->png_done_other = e2; s->state_other = other;
        // from now on the encoder's kernels run NEXT TO the following frame's network, like the look-ahead masks do: the network's
        // persistent grids leave them SIDE_CUS CUs and the generic kernel's hand-off between co-resident blocks is off (timed_conv)
        net_reserve_cus(s->net, SIDE_CUS);
        if (s->img_net) net_reserve_cus(s->img_net, SIDE_CUS);
    }
    FAV_HIP(hipEventRecord(s->ev_png_in, st));                 // the frame is complete at this point of the caller's queue
    FAV_HIP(hipStreamWaitEvent(s->png_q, s->ev_png_in, 0));
    int rc = launch_png_encode(nullptr, s->state, s->Wo, s->Ho, png_out, capacity, png_bytes_out, s->png_ws, s->png_ws_bytes, s->png_q);
    if (rc) return rc;
    FAV_HIP(hipEventRecord(s->png_done, s->png_q));
    s->png_pending = true;
    return FAV_OK;
}

extern "C" int fav_stream_set_host_ordered(fav_stream* s, int on)
{
    FAV_REQUIRE(s, "fav_stream_set_host_ordered: null stream");
    FAV_HIP(hipSetDevice(net_device(s->net)));
    if (on && !s->done_host) {
        FAV_HIP(hipHostMalloc(reinterpret_cast<void**>(&s->done_host), 128, hipHostMallocDefault));
        for (int i = 0; i < 32; ++i) s->done_host[i] = 0u;
        s->retired_host = s->done_host + 16;               // its own 64-byte line
    }
    for (auto& pf : s->pref) { pf.valid = false; pf.retired = 0; }     // look-aheads in flight in the other mode are dropped (their queues drain on their own)
    s->host_ordered = on != 0;
    return FAV_OK;
}

extern "C" int fav_stream_output_size(const fav_stream* s, int* Ho, int* Wo)
{
    FAV_REQUIRE(s && Ho && Wo, "fav_stream_output_size: null argument");
    *Ho = s->Ho; *Wo = s->Wo;
    return FAV_OK;
}

extern "C" int fav_stream_get_input_f32(const fav_stream* s, float* in7, fav_hipstream_t stream)
{
    FAV_REQUIRE(s && in7 && s->frame_counter > 0, "fav_stream_get_input_f32: no frame has been assembled yet");
    FAV_REQUIRE(!s->last_scaled, "fav_stream_get_input_f32: the last frame ran at the scaled single-image size (this view is the H x W input)");
    FAV_HIP(hipSetDevice(net_device(s->net)));
    return launch_unpad_input(s->in8, s->H, s->W, net_pad(s->net), in7, static_cast<hipStream_t>(stream));
}

extern "C" const uint8_t* fav_stream_last_mask(const fav_stream* s) { return s ? s->mask : nullptr; }
