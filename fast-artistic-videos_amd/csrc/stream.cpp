// stream.cpp -- host side of the fused per-frame pipeline: look-ahead masks, host-ordered mode, asynchronous PNG encoding, -scale_factor.
//
// fav_stream: replaces one iteration of run_fast_neural_video's loop (core.lua:194-211) with the video
//             CLI's callbacks (fast_artistic_video.lua:93-172), keeping last_frame_stylized on the device.
//
// The network is opaque here: a stream drives its fav_net through the net_* accessors of fav_internal.h (net.cpp), as vr.cpp does.
#include <algorithm>
#include <cstdlib>

#include <unistd.h>

#include "dev_owned.h"

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
    dev_ptr<float> state;        // last_frame_stylized: [3][Ho][Wo] float RGB, unclamped (fav.lua:169)
    bool has_state = false;
    unsigned frame_counter = 0;  // 1-based index of the frame being stylised (key of the uniform-random fill)
    dev_ptr<float> in8;          // padded NHWC8 network input
    // -scale_factor (fav_stream_set_single_image_size): frames without a prior run at sHs x sWs (0: unscaled).  The scaled padded input
    // and the network's planar output at that size (sHo x sWo) live here from the call that sets the size on
    int sHs = 0, sWs = 0, sHo = 0, sWo = 0;
    dev_ptr<float> scaled_in8, scaled_out;
    bool last_scaled = false;    // the last frame ran at the scaled size: in8 does not hold its input
    dev_ptr<float> cert_tmp, cert;
    dev_ptr<uint8_t> mask;       // certainty as the checker writes it (u8 {0,255})
    dev_ptr<int> q0_main;        // the XCD the caller's queue deals block 0 of a launch to (written by prep_input_kernel, read by the look-ahead mask's long-lived kernels)
    dev_ptr<void> ws; size_t ws_bytes = 0;
    dev_ptr<void> png_ws; size_t png_ws_bytes = 0;        // workspace of fav_stream_encode_png (allocated on first use)
    dev_ptr<uint8_t> color_rgb8;                          // fav_stream_encode_png_colors: the image [Ho][Wo][3] it encodes (allocated on first use)
    // fav_stream_encode_png_async: the encoder's kernels run on a queue of their own, next to the NEXT frame's network (they fill the
    // tails of its grids instead of standing in front of it).  The state is double-buffered from then on: frame i + 1 is written into
    // the other buffer while frame i's is being encoded, and the frame that comes back to a buffer waits for that buffer's encoder
    queue_h png_q; event_h ev_png_in;
    dev_ptr<float> state_other;                           // the buffer `state` is not (null until the first asynchronous encode)
    event_h png_done, png_done_other;                             // the last encode that read `state` / `state_other` ...
    bool png_pending = false, png_pending_other = false;          // ... if nothing has waited for it yet
    // look-ahead mask (fav_stream_prefetch_mask)
    // two side queues with their own structure workspaces: the masks of frames i+1 and i+2 are computed concurrently
    // (each 4-argument mask contains a ~3 ms sequential fp32 chain, CMatrix::avg), three look-ahead slots
    static constexpr int NSIDE = 2, NPREF = 4;
    queue_h side[NSIDE]; dev_ptr<void> side_ws[NSIDE]; event_h ev_in;      // (only the NSIDE_USED queues that can be indexed exist)
    struct Pref { dev_ptr<uint8_t> mask; dev_ptr<float> cert; event_h done; bool valid = false;
                  const void *frame = nullptr, *bw = nullptr, *fw = nullptr; int structure = 0;
                  uint32_t retired = 0; };       // host-ordered: retire sequence of the (mask, cert) buffers now in this slot (0: never read)
    Pref pref[NPREF]; int pref_next = 0, side_next = 0;
    // host-ordered look-ahead (fav_stream_set_host_ordered): no event ever enters the caller's queue or the side queues; a one-thread
    // kernel behind the mask pipeline stores a sequence number into host-mapped memory, which fav_stream_next_frame_flow polls
    bool host_ordered = false;
    host_ptr<uint32_t> done_host;       // [NPREF] (+ retired_host)
    uint32_t pref_seq[NPREF] = {0, 0, 0, 0}; uint32_t seq_counter = 0;
    // ... and nothing orders a side queue behind the caller's queue either, so the buffers a consumed look-ahead swaps OUT of the stream
    // (read by the previous frames' kernels on the caller's queue) must not be rewritten by a later look-ahead before those kernels are
    // through: the consuming call first enqueues a one-thread kernel on the caller's queue that stores a retire sequence number into
    // host-mapped memory (everything enqueued before it has then finished), and a look-ahead into a slot waits ON THE HOST for the
    // sequence number of the buffers it holds (with NPREF slots and two frames of look-ahead that frame finished long ago: no wait)
    uint32_t* retired_host = nullptr; uint32_t retire_counter = 0;      // (a view into done_host's allocation, on its own 64-byte line)
    // long-term priors (fav_stream_set_long_term): the configured distances (ascending, lt_dist[0] == 1) and the HISTORY, a ring of the
    // last lt_dist[lt_n - 1] stylised frames and input frames -- entry of distance d: hist[(hist_head - (d - 1)) mod size], d <= hist_count
    int lt_n = 0; int lt_dist[FAV_LONG_TERM_MAX] = {0, 0, 0, 0};
    struct Hist { dev_ptr<float> state; dev_ptr<uint8_t> frame; bool has_frame = false; };      // (a state set from outside has no frame)
    std::vector<Hist> hist; int hist_head = 0, hist_count = 0;
    dev_ptr<uint8_t> lt_mask[FAV_LONG_TERM_MAX]; dev_ptr<float> lt_cert[FAV_LONG_TERM_MAX];      // per distance beyond the first (that one: mask, cert)
    hipStream_t last_st = nullptr; bool ran = false;       // the HIP stream of the last forward (forgotten by the destructor)
    ~fav_stream()
    {
        if (net) (void)hipSetDevice(net_device(net));
        if (net && ran) net_forget_stream(net, last_st);
        // the one ordering the members' own destruction (reverse declaration order) would not give: the stream's queues are drained and
        // destroyed BEFORE any buffer or host flag their kernels touch is freed, wherever those are declared
        png_q.reset();
        for (auto& q : side) q.reset();
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
static int create_side_stream(queue_h& out)
{
    // (confining the side queues with a CU mask -- hipExtStreamCreateWithCUMask -- measured slower than leaving the CUs free, rounds 2-3)
    // FAV_SIDE_CU_MASK=<comma-separated bit numbers>: experiment, round 6
    if (const char* m = diag_env("FAV_SIDE_CU_MASK")) {
        uint32_t words[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (const char* p = m; *p;) { const int b = atoi(p); if (b >= 0 && b < 256) words[b / 32] |= 1u << (b % 32); while (*p && *p != ',') ++p; if (*p == ',') ++p; }
        hipStream_t q = nullptr;
        FAV_HIP(hipExtStreamCreateWithCUMask(&q, 8, words));
        out.reset(q);
        return FAV_OK;
    }
    return queue_create(out, "side queues");
}

extern "C" int fav_stream_create(fav_net* net, int H, int W, const fav_stream_opts* o, fav_stream** out)
{
    FAV_REQUIRE(net && out && H > 0 && W > 0, "fav_stream_create: bad argument");
    const int pad = net_pad(net);
    FAV_REQUIRE(pad < H && pad < W, "fav_stream_create: %dx%d is smaller than the reflection padding %d", W, H, pad);
    int Ho, Wo; net_out_size(net, H, W, &Ho, &Wo);
    FAV_REQUIRE(Ho >= 1 && Wo >= 1, "frame size %dx%d is too small for the architecture", W, H);
    FAV_HIP(hipSetDevice(net_device(net)));
    std::unique_ptr<fav_stream> s(new fav_stream());      // (every failure below is a plain return: the handles free what exists by then)
    s->net = net; s->H = H; s->W = W; s->Ho = Ho; s->Wo = Wo;
    if (o) s->opts = *o; else { s->opts.border_mode = FAV_BORDER_STN; s->opts.occlusions_min_filter = 7; s->opts.invert_occlusion = 0; s->opts.fix_occlusions = 0; s->opts.fill_random = 0; s->opts.seed = 0; }
    if (s->opts.occlusions_min_filter < 1) s->opts.occlusions_min_filter = 1;
    FAV_REQUIRE(s->opts.occlusions_min_filter <= MIN_FILTER_RMAX, "fav_stream_create: -occlusions_min_filter %d is larger than the supported maximum of %d",
                s->opts.occlusions_min_filter, MIN_FILTER_RMAX);
    const size_t n = (size_t)H * W;
    s->ws_bytes = structure_workspace_bytes(W, H);
    const unsigned ef = hipEventDisableTiming | hipEventDisableSystemFence;
    const char* what = "hipMalloc(stream buffers)";
    if (dev_alloc(s->state, (size_t)3 * Ho * Wo, what) || dev_alloc(s->in8, (size_t)(H + 2 * pad) * (W + 2 * pad) * 8, what) ||
        dev_alloc(s->cert_tmp, n, what) || dev_alloc(s->cert, n, what) || dev_alloc(s->mask, n, what) || dev_alloc(s->q0_main, 16, what) ||
        event_create(s->ev_in, ef, what) || dev_alloc(s->ws, s->ws_bytes, what)) return FAV_EHIP;
    FAV_HIP(hipMemset(s->q0_main.get(), 0, 16 * sizeof(int)));
    for (auto& pf : s->pref)
        if (dev_alloc(pf.mask, n, "look-ahead slots") || dev_alloc(pf.cert, n, "look-ahead slots") || event_create(pf.done, ef, "look-ahead slots")) return FAV_EHIP;
    // the side queues a look-ahead can ever be dealt to (fav_stream_prefetch_mask: q < NSIDE_USED), each with its structure workspace
    for (int i = 0; i < NSIDE_USED; ++i)
        if (create_side_stream(s->side[i]) || dev_alloc(s->side_ws[i], s->ws_bytes, "side queues")) return FAV_EHIP;
    *out = s.release();
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
    if (s->png_pending) { FAV_HIP(hipStreamWaitEvent(st, s->png_done.get(), 0)); s->png_pending = false; }
    return FAV_OK;
}

// the forward that was to fill the buffer state_for_writing() switched to has failed: `state` names the last COMPLETE frame again
static void state_writing_failed(fav_stream* s)
{
    if (!s->state_other) return;
    swap_state_buffers(s);
}

// long-term priors: the current state, and the frame it was stylised from (null: a state set from outside), become the history's newest entry
static int history_push(fav_stream* s, const uint8_t* frame, hipStream_t st)
{
    const int size = (int)s->hist.size();
    s->hist_head = s->hist_count ? (s->hist_head + 1) % size : 0;
    fav_stream::Hist& h = s->hist[s->hist_head];
    FAV_HIP(hipMemcpyAsync(h.state.get(), s->state.get(), (size_t)3 * s->Ho * s->Wo * 4, hipMemcpyDeviceToDevice, st));
    if (frame) FAV_HIP(hipMemcpyAsync(h.frame.get(), frame, (size_t)3 * s->H * s->W, hipMemcpyDeviceToDevice, st));
    h.has_frame = frame != nullptr;
    s->hist_count = std::min(s->hist_count + 1, size);
    return FAV_OK;
}

static const fav_stream::Hist& history_at(const fav_stream* s, int distance)
{
    const int size = (int)s->hist.size();
    return s->hist[((s->hist_head - (distance - 1)) % size + size) % size];
}

// how many of the configured distances, from the first, the history serves (with_frames: ... and holds the input frame of)
static int history_available(const fav_stream* s, bool with_frames)
{
    int m = 0;
    while (m < s->lt_n && s->lt_dist[m] <= s->hist_count && (!with_frames || history_at(s, s->lt_dist[m]).has_frame)) ++m;
    return m;
}

static int stream_finish(fav_stream* s, const uint8_t* frame, float* out_rgb_f32, uint8_t* out_rgb8_hwc, hipStream_t st)
{
    const size_t n = (size_t)s->Ho * s->Wo;
    s->has_state = true;
    if (s->lt_n) { int rc = history_push(s, frame, st); if (rc) return rc; }
    if (out_rgb_f32) FAV_HIP(hipMemcpyAsync(out_rgb_f32, s->state.get(), 3 * n * 4, hipMemcpyDeviceToDevice, st));
    if (out_rgb8_hwc) return launch_quantize_rgb8(s->state.get(), out_rgb8_hwc, s->Ho, s->Wo, st);
    return FAV_OK;
}

extern "C" int fav_stream_first_frame(fav_stream* s, const uint8_t* frame_rgb_hwc, float* out_rgb_f32, uint8_t* out_rgb8_hwc,
                                      fav_hipstream_t stream)
{
    FAV_REQUIRE(s && frame_rgb_hwc, "fav_stream_first_frame: null argument");
    FAV_HIP(hipSetDevice(net_device(s->net)));
    hipStream_t st = static_cast<hipStream_t>(stream);
    ++s->frame_counter;
    s->hist_count = 0;                                   // long-term priors: nothing from before a frame without a prior is warped in
    fav_net* fn = s->img_net ? s->img_net : s->net;      // image model: 3 content channels (the zero prior / mask planes meet zero weights)
    if (s->sHs) {      // core.lua:127-130,150-152: resampled before the model, the result resampled back to H x W (= Ho x Wo) into the state
        int rc = launch_scale_prep(frame_rgb_hwc, s->H, s->W, s->sHs, s->sWs, net_pad(s->net), s->scaled_in8.get(), st,
                                   s->img_net ? 0 : s->opts.fill_random, s->opts.seed, s->frame_counter);
        if (rc) return rc;
        s->last_st = st; s->ran = true; s->last_scaled = true;
        rc = state_for_writing(s, st); if (rc) return rc;
        rc = net_forward_padded(fn, s->scaled_in8.get(), s->sHs, s->sWs, s->scaled_out.get(), st);
        if (!rc) rc = launch_scale_planar(s->scaled_out.get(), s->state.get(), 3, s->sHo, s->sWo, s->Ho, s->Wo, st);
        if (rc) { state_writing_failed(s); return rc; }
        return stream_finish(s, frame_rgb_hwc, out_rgb_f32, out_rgb8_hwc, st);
    }
    // the image model sees only the three content channels (core.lua:146): no fill there
    int rc = launch_prep_input(frame_rgb_hwc, nullptr, 0, 0, nullptr, nullptr, s->opts.border_mode, s->H, s->W, net_pad(s->net), s->in8.get(), st,
                               s->img_net ? 0 : s->opts.fill_random, s->opts.seed, s->frame_counter);
    if (rc) return rc;
    s->last_st = st; s->ran = true; s->last_scaled = false;
    rc = state_for_writing(s, st); if (rc) return rc;
    rc = net_forward_padded(fn, s->in8.get(), s->H, s->W, s->state.get(), st); if (rc) { state_writing_failed(s); return rc; }
    return stream_finish(s, frame_rgb_hwc, out_rgb_f32, out_rgb8_hwc, st);
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
    if (Hs == 0 && Ws == 0) {      // back to the unscaled path (freeing waits for the frames that still read the buffers)
        s->scaled_in8.reset(); s->scaled_out.reset();
        s->sHs = s->sWs = s->sHo = s->sWo = 0;
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
    dev_ptr<float> in8, out;      // both or neither: the stream keeps its old pair when either allocation fails
    const char* what = "hipMalloc(scaled single-image buffers)";
    if (dev_alloc(in8, (size_t)(Hs + 2 * pad) * (Ws + 2 * pad) * 8, what) || dev_alloc(out, (size_t)3 * Ho * Wo, what)) return FAV_EHIP;
    s->scaled_in8 = std::move(in8); s->scaled_out = std::move(out); s->sHs = Hs; s->sWs = Ws; s->sHo = Ho; s->sWo = Wo;      // (freeing the old pair waits for the frames that still read it)
    return FAV_OK;
}

// host-ordered mode: the HOST waits until done() sees the sequence number that a one-thread kernel on queue `q` stores into host-mapped
// memory, and asks the queue every 2048 spins (0.1 s) whether it has failed (`what` names it in the error text)
template <class Done> static int host_wait(Done done, hipStream_t q, const char* what)
{
    for (int spins = 0; !done(); ++spins) {
        usleep(50);
        if ((spins & 2047) == 2047) { const hipError_t e = hipStreamQuery(q); if (e != hipSuccess && e != hipErrorNotReady) return hip_fail(e, what); }
    }
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
                                     s->opts.occlusions_min_filter, s->cert_tmp.get(), s->cert.get(), s->H, s->W, st);
        if (rc) return rc;
        ++s->frame_counter;
        rc = launch_prep_input(frame, s->state.get(), s->Ho, s->Wo, bw, s->cert.get(), s->opts.border_mode, s->H, s->W, net_pad(s->net), s->in8.get(), st,
                               s->opts.fill_random, s->opts.seed, s->frame_counter, s->q0_main.get());
        if (rc) return rc;
    }
    s->last_st = st; s->ran = true; s->last_scaled = false;
    rc = state_for_writing(s, st); if (rc) return rc;       // (the prior was read from the previous state above)
    { TraceRange tr_net("fav:network"); rc = net_forward_padded(s->net, s->in8.get(), s->H, s->W, s->state.get(), st); }
    if (rc) { state_writing_failed(s); return rc; }
    return stream_finish(s, frame, out_f32, out_u8, st);
}

extern "C" int fav_stream_next_frame_cert(fav_stream* s, const uint8_t* frame_rgb_hwc, const float* backward_flo,
                                          const uint8_t* cert_pgm, float* out_rgb_f32, uint8_t* out_rgb8_hwc,
                                          fav_hipstream_t stream)
{
    FAV_REQUIRE(s && frame_rgb_hwc && backward_flo && cert_pgm, "fav_stream_next_frame_cert: null argument");
    FAV_HIP(hipSetDevice(net_device(s->net)));
    hipStream_t st = static_cast<hipStream_t>(stream);
    FAV_HIP(hipMemcpyAsync(s->mask.get(), cert_pgm, (size_t)s->H * s->W, hipMemcpyDeviceToDevice, st));
    return stream_next(s, frame_rgb_hwc, backward_flo, s->mask.get(), out_rgb_f32, out_rgb8_hwc, st);
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
                volatile uint32_t* flag = s->done_host.get() + slot;
                int rcw = host_wait([&] { return *flag == s->pref_seq[slot]; }, s->side[0].get(), "look-ahead queue"); if (rcw) return rcw;
                // the buffers about to leave the stream were read by kernels already in the caller's queue: mark the point behind them
                pf.retired = ++s->retire_counter;
                int rcf = launch_store_flag(s->retired_host, pf.retired, st); if (rcf) return rcf;
            } else FAV_HIP(hipStreamWaitEvent(st, pf.done.get(), 0));
            std::swap(s->mask, pf.mask);
            std::swap(s->cert, pf.cert);          // mask -> certainty (options, erosion) was done on the side queue as well
            return stream_next(s, frame_rgb_hwc, backward_flo, s->mask.get(), out_rgb_f32, out_rgb8_hwc, st, true);
        }
    // not prefetched: compute inline on the caller's stream (own workspace)
    TraceRange tr_mask("fav:consistency mask");
    const float* structure = nullptr; const float* avg = nullptr;
    if (use_structure) {
        int rc = launch_structure(frame_rgb_hwc, s->W, s->H, s->ws.get(), s->ws_bytes, &structure, &avg, st); if (rc) return rc;
    }
    // check + certainty options + erosion + input assembly in ONE tile kernel (round 5; the mask byte and the eroded certainty of every pixel
    // are still written: fav_stream_last_mask); FAV_NO_CHECK_PREP: the check and the assembly as two launches (rounds 3-4)
    static const bool fused_prep = diag_env("FAV_NO_CHECK_PREP") == nullptr;      // (tuning: read once)
    if (fused_prep && s->has_state) {
        ++s->frame_counter;
        int rcp = launch_check_prep(frame_rgb_hwc, s->state.get(), s->Ho, s->Wo, backward_flo, forward_flo, structure, avg, s->mask.get(), s->cert.get(),
                                    s->opts.invert_occlusion, s->opts.fix_occlusions, s->opts.border_mode, s->opts.occlusions_min_filter,
                                    s->H, s->W, net_pad(s->net), s->in8.get(), st, s->opts.fill_random, s->opts.seed, s->frame_counter);
        if (rcp) return rcp;
        return stream_next(s, frame_rgb_hwc, backward_flo, s->mask.get(), out_rgb_f32, out_rgb8_hwc, st, true, true);
    }
    int rc = launch_check_cert(backward_flo, forward_flo, structure, avg, s->mask.get(), s->opts.invert_occlusion, s->opts.fix_occlusions, s->opts.border_mode,
                               s->opts.occlusions_min_filter, s->cert.get(), s->H, s->W, st);
    if (rc) return rc;
    return stream_next(s, frame_rgb_hwc, backward_flo, s->mask.get(), out_rgb_f32, out_rgb8_hwc, st, true);
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
    const fav_flow_opts_ex3 ex3 = flow_opts_no_median(flow_opts_host);
    return fav_stream_next_frame_estimate_ex3(s, frame_rgb_hwc, prev_frame_rgb_hwc, &ex3, use_structure, backward_flo, forward_flo, workspace, workspace_bytes,
                                              out_rgb_f32, out_rgb8_hwc, stream);
}

extern "C" int fav_stream_next_frame_estimate_ex3(fav_stream* s, const uint8_t* frame_rgb_hwc, const uint8_t* prev_frame_rgb_hwc,
                                                  const fav_flow_opts_ex3* flow_opts_host, int use_structure, float* backward_flo, float* forward_flo,
                                                  void* workspace, size_t workspace_bytes, float* out_rgb_f32, uint8_t* out_rgb8_hwc,
                                                  fav_hipstream_t stream)
{
    FAV_REQUIRE(s && frame_rgb_hwc && prev_frame_rgb_hwc && backward_flo && forward_flo, "fav_stream_next_frame_estimate: null argument");
    FAV_HIP(hipSetDevice(net_device(s->net)));
    const size_t pair_bytes = fav_flow_pairs_workspace_bytes_ex3(s->W, s->H, 1, flow_opts_host);      // (0: a bad option; the single call reports it)
    int rc;
    if (pair_bytes && workspace_bytes >= pair_bytes) {
        rc = fav_flow_pairs_rgb8_ex3(&prev_frame_rgb_hwc, &frame_rgb_hwc, 1, s->W, s->H, flow_opts_host, &backward_flo, &forward_flo, workspace,
                                     workspace_bytes, stream);
        if (rc) return rc;
    } else {
        rc = fav_flow_rgb8_ex3(frame_rgb_hwc, prev_frame_rgb_hwc, s->W, s->H, flow_opts_host, backward_flo, workspace, workspace_bytes, stream);
        if (rc) return rc;
        rc = fav_flow_rgb8_ex3(prev_frame_rgb_hwc, frame_rgb_hwc, s->W, s->H, flow_opts_host, forward_flo, workspace, workspace_bytes, stream);
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
    hipStream_t sd = s->side[q].get();
    if (!s->host_ordered) {
        FAV_HIP(hipEventRecord(s->ev_in.get(), st));                 // inputs are complete at this point of the caller's stream
        FAV_HIP(hipStreamWaitEvent(sd, s->ev_in.get(), 0));          // (work enqueued on `stream` AFTER this call is not waited for)
    } else if (pf.retired) {                                   // host-ordered: the caller has SEEN the inputs complete (fav.h) ...
        // ... and the slot's buffers were read by frames on the caller's queue: those must be through before a side queue rewrites them
        volatile uint32_t* flag = s->retired_host;
        int rcw = host_wait([&] { return (int32_t)(*flag - pf.retired) >= 0; }, st, "look-ahead: the caller's queue"); if (rcw) return rcw;
        pf.retired = 0;
    }
    const float* structure = nullptr; const float* avg = nullptr;
    if (use_structure) {
        int rc = launch_structure(frame_rgb_hwc, s->W, s->H, s->side_ws[q].get(), s->ws_bytes, &structure, &avg, sd, SIDE_PACK >= 0 ? SIDE_PACK : SIDE_CUS, s->q0_main.get()); if (rc) return rc;
    }
    // mask + certainty of the frame (mask options, fix_occlusions warp of ones, erosion): depends on the flows and the stream's options only
    int rc = launch_check_cert(backward_flo, forward_flo, structure, avg, pf.mask.get(), s->opts.invert_occlusion, s->opts.fix_occlusions, s->opts.border_mode,
                               s->opts.occlusions_min_filter, pf.cert.get(), s->H, s->W, sd);
    if (rc) return rc;
    if (s->host_ordered) {
        const int slot = (int)(&pf - s->pref);
        s->pref_seq[slot] = ++s->seq_counter;
        rc = launch_store_flag(s->done_host.get() + slot, s->pref_seq[slot], sd); if (rc) return rc;
    } else FAV_HIP(hipEventRecord(pf.done.get(), sd));
    pf.valid = true; pf.frame = frame_rgb_hwc; pf.bw = backward_flo; pf.fw = forward_flo; pf.structure = use_structure != 0;
    return FAV_OK;
}

extern "C" int fav_stream_get_state(fav_stream* s, float* state_rgb_f32, fav_hipstream_t stream)
{
    FAV_REQUIRE(s && state_rgb_f32 && s->has_state, "fav_stream_get_state: no state");
    FAV_HIP(hipSetDevice(net_device(s->net)));
    FAV_HIP(hipMemcpyAsync(state_rgb_f32, s->state.get(), (size_t)3 * s->Ho * s->Wo * 4, hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)));
    return FAV_OK;
}

extern "C" int fav_stream_set_state(fav_stream* s, const float* state_rgb_f32, fav_hipstream_t stream)
{
    FAV_REQUIRE(s && state_rgb_f32, "fav_stream_set_state: null argument");
    FAV_HIP(hipSetDevice(net_device(s->net)));
    if (s->png_pending) { FAV_HIP(hipStreamWaitEvent(static_cast<hipStream_t>(stream), s->png_done.get(), 0)); s->png_pending = false; }
    FAV_HIP(hipMemcpyAsync(s->state.get(), state_rgb_f32, (size_t)3 * s->Ho * s->Wo * 4, hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)));
    s->has_state = true;
    s->hist_count = 0;                                   // long-term priors: the history restarts with this state (it has no frame)
    if (s->lt_n) return history_push(s, nullptr, static_cast<hipStream_t>(stream));
    return FAV_OK;
}

extern "C" int fav_stream_wait_png(fav_stream* s, fav_hipstream_t stream)
{
    FAV_REQUIRE(s, "fav_stream_wait_png: null stream");
    FAV_HIP(hipSetDevice(net_device(s->net)));
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (s->png_pending) FAV_HIP(hipStreamWaitEvent(st, s->png_done.get(), 0));
    if (s->png_pending_other) FAV_HIP(hipStreamWaitEvent(st, s->png_done_other.get(), 0));
    return FAV_OK;
}

// the encoder's workspace, allocated on first use (both encode calls share the one)
static int ensure_png_ws(fav_stream* s)
{
    if (s->png_ws) return FAV_OK;
    s->png_ws_bytes = png_workspace_bytes(s->Wo, s->Ho);
    return dev_alloc(s->png_ws, s->png_ws_bytes);
}

extern "C" int fav_stream_encode_png(fav_stream* s, void* png_out, size_t capacity, uint32_t* png_bytes_out, fav_hipstream_t stream)
{
    FAV_REQUIRE(s && s->has_state, "fav_stream_encode_png: no stylised frame yet");
    FAV_HIP(hipSetDevice(net_device(s->net)));
    { int rc = ensure_png_ws(s); if (rc) return rc; }
    if (s->png_q) { int rc = fav_stream_wait_png(s, stream); if (rc) return rc; }      // (one workspace: behind the asynchronous encodes)
    return launch_png_encode(nullptr, s->state.get(), s->Wo, s->Ho, png_out, capacity, png_bytes_out, s->png_ws.get(), s->png_ws_bytes, static_cast<hipStream_t>(stream));
}

// the current stylised frame as the planes of a YUV4MPEG2 frame (kernels_yuv.hip): one launch on the caller's queue, no workspace
extern "C" int fav_stream_encode_yuv(fav_stream* s, const fav_yuv_format* fmt_host, uint8_t* yuv_out, size_t capacity, fav_hipstream_t stream)
{
    FAV_REQUIRE(s && s->has_state, "fav_stream_encode_yuv: no stylised frame yet");
    FAV_REQUIRE(yuv_out, "fav_stream_encode_yuv: null output");
    { int rc = yuv_format_check("fav_stream_encode_yuv", s->Wo, s->Ho, fmt_host); if (rc) return rc; }
    const size_t need = yuv_frame_bytes(s->Wo, s->Ho, *fmt_host);
    FAV_REQUIRE(capacity >= need, "fav_stream_encode_yuv: a %dx%d frame takes %zu bytes, the buffer holds %zu", s->Wo, s->Ho, need, capacity);
    FAV_HIP(hipSetDevice(net_device(s->net)));
    return launch_rgb_to_yuv(nullptr, s->state.get(), s->Wo, s->Ho, *fmt_host, yuv_out, static_cast<hipStream_t>(stream));
}

// the same for every layout of include/fav_yuv.h (kernels_yuv_layout.hip): above 8 bits the state's floats enter unquantised
extern "C" int fav_stream_encode_yuv_layout(fav_stream* s, const fav_yuv_layout* layout_host, void* yuv_out, size_t capacity, fav_hipstream_t stream)
{
    FAV_REQUIRE(s && s->has_state, "fav_stream_encode_yuv_layout: no stylised frame yet");
    FAV_REQUIRE(yuv_out, "fav_stream_encode_yuv_layout: null output");
    { int rc = yuv_layout_check("fav_stream_encode_yuv_layout", s->Wo, s->Ho, layout_host); if (rc) return rc; }
    const size_t need = yuv_layout_frame_bytes(s->Wo, s->Ho, *layout_host);
    FAV_REQUIRE(capacity >= need, "fav_stream_encode_yuv_layout: a %dx%d frame takes %zu bytes, the buffer holds %zu", s->Wo, s->Ho, need, capacity);
    FAV_HIP(hipSetDevice(net_device(s->net)));
    return launch_rgb_to_yuv_layout(nullptr, s->state.get(), s->Wo, s->Ho, *layout_host, yuv_out, static_cast<hipStream_t>(stream));
}

// -original_colors: the current stylised frame's luminance on the colours of `frame_rgb_hwc` (kernels_color.hip).  The state is read only.
// The frame and the stylised frame must be one size: a network that pads its output to a multiple of 4 has no original pixel there
static int colors_size_check(const char* who, const fav_stream* s)
{
    if (s->Wo == s->W && s->Ho == s->H) return FAV_OK;
    set_error("%s: the stylised frames are %dx%d, the original frames %dx%d: the colours of one cannot be laid over the other", who, s->Wo, s->Ho, s->W, s->H);
    return FAV_EUNSUPPORTED;
}

extern "C" int fav_stream_encode_png_colors(fav_stream* s, const uint8_t* frame_rgb_hwc, int matrix, void* png_out, size_t capacity,
                                            uint32_t* png_bytes_out, fav_hipstream_t stream)
{
    FAV_REQUIRE(s && s->has_state, "fav_stream_encode_png_colors: no stylised frame yet");
    FAV_REQUIRE(frame_rgb_hwc && png_out && png_bytes_out, "fav_stream_encode_png_colors: null pointer");
    FAV_REQUIRE(matrix == FAV_YUV_BT601 || matrix == FAV_YUV_BT709, "fav_stream_encode_png_colors: matrix must be 0 (BT.601) or 1 (BT.709), not %d", matrix);
    { int rc = colors_size_check("fav_stream_encode_png_colors", s); if (rc) return rc; }
    FAV_REQUIRE(capacity >= png_capacity(s->Wo, s->Ho), "fav_stream_encode_png_colors: output capacity %zu < fav_png_capacity = %zu", capacity, png_capacity(s->Wo, s->Ho));
    FAV_HIP(hipSetDevice(net_device(s->net)));
    hipStream_t st = static_cast<hipStream_t>(stream);
    { int rc = ensure_png_ws(s); if (rc) return rc; }
    if (!s->color_rgb8) { int rc = dev_alloc(s->color_rgb8, (size_t)3 * s->Ho * s->Wo, "fav_stream_encode_png_colors: image buffer"); if (rc) return rc; }
    if (s->png_q) { int rc = fav_stream_wait_png(s, stream); if (rc) return rc; }      // (one workspace: behind the asynchronous encodes)
    int rc = launch_color_transfer_rgb8(s->state.get(), frame_rgb_hwc, s->Wo, s->Ho, matrix, s->color_rgb8.get(), st); if (rc) return rc;
    return launch_png_encode(s->color_rgb8.get(), nullptr, s->Wo, s->Ho, png_out, capacity, png_bytes_out, s->png_ws.get(), s->png_ws_bytes, st);
}

extern "C" int fav_stream_encode_yuv_colors(fav_stream* s, const uint8_t* frame_rgb_hwc, const fav_yuv_format* fmt_host, uint8_t* yuv_out,
                                            size_t capacity, fav_hipstream_t stream)
{
    FAV_REQUIRE(s && s->has_state, "fav_stream_encode_yuv_colors: no stylised frame yet");
    FAV_REQUIRE(frame_rgb_hwc && yuv_out, "fav_stream_encode_yuv_colors: null pointer");
    { int rc = yuv_format_check("fav_stream_encode_yuv_colors", s->Wo, s->Ho, fmt_host); if (rc) return rc; }
    { int rc = colors_size_check("fav_stream_encode_yuv_colors", s); if (rc) return rc; }
    const size_t need = yuv_frame_bytes(s->Wo, s->Ho, *fmt_host);
    FAV_REQUIRE(capacity >= need, "fav_stream_encode_yuv_colors: a %dx%d frame takes %zu bytes, the buffer holds %zu", s->Wo, s->Ho, need, capacity);
    FAV_HIP(hipSetDevice(net_device(s->net)));
    return launch_color_transfer_yuv(s->state.get(), frame_rgb_hwc, s->Wo, s->Ho, *fmt_host, yuv_out, static_cast<hipStream_t>(stream));
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
        const char* what = "fav_stream_encode_png_async: encoder queue / second state buffer";
        queue_h q; event_h e0, e1, e2; dev_ptr<float> other;
        if (queue_create(q, what) || event_create(e0, ef, what) || event_create(e1, ef, what) || event_create(e2, ef, what) ||
            dev_alloc(other, (size_t)3 * s->Ho * s->Wo, what)) return FAV_EHIP;
        s->png_q = std::move(q); s->ev_png_in = std::move(e0); s->png_done = std::move(e1); s->png_done_other = std::move(e2); s->state_other = std::move(other);
        // from now on the encoder's kernels run NEXT TO the following frame's network, like the look-ahead masks do: the network's
        // persistent grids leave them SIDE_CUS CUs and the generic kernel's hand-off between co-resident blocks is off (timed_conv)
        net_reserve_cus(s->net, SIDE_CUS);
        if (s->img_net) net_reserve_cus(s->img_net, SIDE_CUS);
    }
    FAV_HIP(hipEventRecord(s->ev_png_in.get(), st));                 // the frame is complete at this point of the caller's queue
    FAV_HIP(hipStreamWaitEvent(s->png_q.get(), s->ev_png_in.get(), 0));
    int rc = launch_png_encode(nullptr, s->state.get(), s->Wo, s->Ho, png_out, capacity, png_bytes_out, s->png_ws.get(), s->png_ws_bytes, s->png_q.get());
    if (rc) return rc;
    FAV_HIP(hipEventRecord(s->png_done.get(), s->png_q.get()));
    s->png_pending = true;
    return FAV_OK;
}

extern "C" int fav_stream_set_host_ordered(fav_stream* s, int on)
{
    FAV_REQUIRE(s, "fav_stream_set_host_ordered: null stream");
    FAV_HIP(hipSetDevice(net_device(s->net)));
    if (on && !s->done_host) {
        int rc = host_alloc(s->done_host, 32, hipHostMallocDefault); if (rc) return rc;
        for (int i = 0; i < 32; ++i) s->done_host.get()[i] = 0u;
        s->retired_host = s->done_host.get() + 16;         // its own 64-byte line
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
    return launch_unpad_input(s->in8.get(), s->H, s->W, net_pad(s->net), in7, static_cast<hipStream_t>(stream));
}

extern "C" int fav_stream_get_padded_input_f32(const fav_stream* s, float* out, fav_hipstream_t stream)
{
    FAV_REQUIRE(s && out && s->frame_counter > 0, "fav_stream_get_padded_input_f32: no frame has been assembled yet");
    FAV_REQUIRE(!s->last_scaled, "fav_stream_get_padded_input_f32: the last frame ran at the scaled single-image size (this view is the H x W input)");
    FAV_HIP(hipSetDevice(net_device(s->net)));
    const int pad = net_pad(s->net);
    FAV_HIP(hipMemcpyAsync(out, s->in8.get(), (size_t)(s->H + 2 * pad) * (s->W + 2 * pad) * 8 * sizeof(float), hipMemcpyDeviceToDevice,
                           static_cast<hipStream_t>(stream)));
    return FAV_OK;
}

extern "C" const uint8_t* fav_stream_last_mask(const fav_stream* s) { return s ? s->mask.get() : nullptr; }

// ================================================================================================
// long-term priors (include/fav_long_term.h; DESIGN.md, "Long-term priors")
// ================================================================================================
extern "C" int fav_stream_set_long_term(fav_stream* s, const int* distances_host, int n)
{
    FAV_REQUIRE(s, "fav_stream_set_long_term: null stream");
    FAV_REQUIRE(n >= 0 && n <= FAV_LONG_TERM_MAX, "fav_stream_set_long_term: %d distances (0 = off, at most %d, distance 1 included)", n, FAV_LONG_TERM_MAX);
    FAV_REQUIRE(n == 0 || distances_host, "fav_stream_set_long_term: null distances");
    for (int k = 0; k < n; ++k) {
        if (k == 0) FAV_REQUIRE(distances_host[0] == 1, "fav_stream_set_long_term: the first distance is %d, it must be 1", distances_host[0]);
        else FAV_REQUIRE(distances_host[k] > distances_host[k - 1], "fav_stream_set_long_term: distance %d follows %d (strictly ascending)", distances_host[k], distances_host[k - 1]);
        FAV_REQUIRE(distances_host[k] <= FAV_LONG_TERM_MAX_DISTANCE, "fav_stream_set_long_term: distance %d is larger than the supported maximum of %d", distances_host[k], FAV_LONG_TERM_MAX_DISTANCE);
    }
    FAV_HIP(hipSetDevice(net_device(s->net)));
    // everything new first: the stream keeps what it has when an allocation fails
    std::vector<fav_stream::Hist> hist(n ? distances_host[n - 1] : 0);
    dev_ptr<uint8_t> mask[FAV_LONG_TERM_MAX]; dev_ptr<float> cert[FAV_LONG_TERM_MAX];
    const size_t px = (size_t)s->H * s->W;
    const char* what = "fav_stream_set_long_term: history";
    for (auto& h : hist)
        if (dev_alloc(h.state, (size_t)3 * s->Ho * s->Wo, what) || dev_alloc(h.frame, 3 * px, what)) return FAV_EHIP;
    for (int k = 1; k < n; ++k)
        if (dev_alloc(mask[k], px, what) || dev_alloc(cert[k], px, what)) return FAV_EHIP;
    s->hist = std::move(hist);                          // (freeing the old buffers waits for the frames that still read them)
    for (int k = 0; k < FAV_LONG_TERM_MAX; ++k) { s->lt_mask[k] = std::move(mask[k]); s->lt_cert[k] = std::move(cert[k]); s->lt_dist[k] = k < n ? distances_host[k] : 0; }
    s->lt_n = n; s->hist_head = 0; s->hist_count = 0;
    // the state the stream already has starts the history, as fav_stream_set_state would (no queue is given here: behind everything the device has been given)
    if (n && s->has_state) {
        FAV_HIP(hipDeviceSynchronize());
        FAV_HIP(hipMemcpy(s->hist[0].state.get(), s->state.get(), (size_t)3 * s->Ho * s->Wo * 4, hipMemcpyDeviceToDevice));
        s->hist[0].has_frame = false; s->hist_count = 1;
    }
    return FAV_OK;
}

extern "C" int fav_stream_long_term_available(const fav_stream* s) { return s ? history_available(s, false) : 0; }

extern "C" int fav_stream_next_frame_flows_lt(fav_stream* s, const uint8_t* frame_rgb_hwc, int m, const float* const* backward_flo,
                                              const float* const* forward_flo, int use_structure, float* out_rgb_f32, uint8_t* out_rgb8_hwc,
                                              fav_hipstream_t stream)
{
    FAV_REQUIRE(s && frame_rgb_hwc && backward_flo && forward_flo, "fav_stream_next_frame_flows_lt: null argument");
    FAV_REQUIRE(s->lt_n > 0, "fav_stream_next_frame_flows_lt: long-term priors are off (fav_stream_set_long_term)");
    const int avail = history_available(s, false);
    FAV_REQUIRE(m >= 1 && m <= avail, "fav_stream_next_frame_flows_lt: flows of %d distances, the history serves %d of the %d configured", m, avail, s->lt_n);
    for (int k = 0; k < m; ++k)
        FAV_REQUIRE(backward_flo[k] && forward_flo[k], "fav_stream_next_frame_flows_lt: null flow for distance %d", s->lt_dist[k]);
    for (auto& pf : s->pref)
        FAV_REQUIRE(!pf.valid, "fav_stream_next_frame_flows_lt: a look-ahead mask (fav_stream_prefetch_mask) is pending; the long-term path does not consume it");
    FAV_REQUIRE(s->has_state, "fav_stream_next_frame_flows_lt: no previous stylised frame");
    FAV_REQUIRE(s->opts.occlusions_min_filter <= MIN_FILTER_RMAX, "fav_stream_next_frame_flows_lt: window %d unsupported", s->opts.occlusions_min_filter);
    FAV_HIP(hipSetDevice(net_device(s->net)));
    hipStream_t st = static_cast<hipStream_t>(stream);
    {
        TraceRange tr_mask("fav:long-term masks + assemble");
        // the 4-argument structure map depends on THIS frame alone (launch_structure reads nothing else): once for all distances
        const float* structure = nullptr; const float* avg = nullptr;
        if (use_structure) { int rc = launch_structure(frame_rgb_hwc, s->W, s->H, s->ws.get(), s->ws_bytes, &structure, &avg, st); if (rc) return rc; }
        const float* states[FAV_LONG_TERM_MAX]; const float* certs[FAV_LONG_TERM_MAX];
        for (int k = 0; k < m; ++k) {
            uint8_t* mask = k ? s->lt_mask[k].get() : s->mask.get();        // (fav_stream_last_mask stays the distance-1 mask)
            float* cert = k ? s->lt_cert[k].get() : s->cert.get();
            int rc = launch_check_cert(backward_flo[k], forward_flo[k], structure, avg, mask, s->opts.invert_occlusion, s->opts.fix_occlusions,
                                       s->opts.border_mode, s->opts.occlusions_min_filter, cert, s->H, s->W, st);
            if (rc) return rc;
            states[k] = history_at(s, s->lt_dist[k]).state.get(); certs[k] = cert;
        }
        ++s->frame_counter;
        int rc = launch_longterm_prep(frame_rgb_hwc, m, states, s->Ho, s->Wo, backward_flo, certs, s->opts.border_mode, s->H, s->W, net_pad(s->net),
                                      s->in8.get(), nullptr, st, s->opts.fill_random, s->opts.seed, s->frame_counter);
        if (rc) return rc;
    }
    return stream_next(s, frame_rgb_hwc, backward_flo[0], s->mask.get(), out_rgb_f32, out_rgb8_hwc, st, true, true);
}

static size_t lt_flow_bytes(const fav_stream* s) { return ((size_t)s->H * s->W * 8 + 255) / 256 * 256; }

extern "C" size_t fav_stream_long_term_workspace_bytes(const fav_stream* s, const fav_flow_opts_ex3* opts_host)
{
    if (!s || s->lt_n == 0) { set_error("fav_stream_long_term_workspace_bytes: long-term priors are off (fav_stream_set_long_term)"); return 0; }
    const size_t pairs = fav_flow_pairs_workspace_bytes_ex3(s->W, s->H, s->lt_n, opts_host);      // (0: a bad option or size, with its message)
    return pairs ? (size_t)2 * s->lt_n * lt_flow_bytes(s) + pairs : 0;
}

extern "C" int fav_stream_next_frame_estimate_lt(fav_stream* s, const uint8_t* frame_rgb_hwc, const fav_flow_opts_ex3* opts_host, int use_structure,
                                                 void* workspace, size_t workspace_bytes, float* out_rgb_f32, uint8_t* out_rgb8_hwc,
                                                 fav_hipstream_t stream)
{
    FAV_REQUIRE(s && frame_rgb_hwc && workspace, "fav_stream_next_frame_estimate_lt: null argument");
    FAV_REQUIRE(s->lt_n > 0, "fav_stream_next_frame_estimate_lt: long-term priors are off (fav_stream_set_long_term)");
    const int m = history_available(s, true);
    FAV_REQUIRE(m >= 1, "fav_stream_next_frame_estimate_lt: the history holds no previous frame (after fav_stream_set_state the first frame takes "
                        "fav_stream_next_frame_estimate_ex3, which is given one)");
    for (auto& pf : s->pref)
        FAV_REQUIRE(!pf.valid, "fav_stream_next_frame_estimate_lt: a look-ahead mask (fav_stream_prefetch_mask) is pending; the long-term path does not consume it");
    const size_t need = fav_stream_long_term_workspace_bytes(s, opts_host);
    if (!need) return FAV_EINVAL;
    FAV_REQUIRE(workspace_bytes >= need, "fav_stream_next_frame_estimate_lt: the workspace holds %zu bytes, fav_stream_long_term_workspace_bytes = %zu", workspace_bytes, need);
    FAV_REQUIRE(((uintptr_t)workspace & 255) == 0, "fav_stream_next_frame_estimate_lt: the workspace is not 256-byte aligned");
    const size_t F = lt_flow_bytes(s);
    char* base = static_cast<char*>(workspace);
    const uint8_t* prev[FAV_LONG_TERM_MAX]; const uint8_t* cur[FAV_LONG_TERM_MAX]; float* bw[FAV_LONG_TERM_MAX]; float* fw[FAV_LONG_TERM_MAX];
    for (int k = 0; k < m; ++k) {
        prev[k] = history_at(s, s->lt_dist[k]).frame.get(); cur[k] = frame_rgb_hwc;
        bw[k] = reinterpret_cast<float*>(base + (size_t)2 * k * F); fw[k] = reinterpret_cast<float*>(base + (size_t)(2 * k + 1) * F);
    }
    const size_t off = (size_t)2 * s->lt_n * F;
    int rc = fav_flow_pairs_rgb8_ex3(prev, cur, m, s->W, s->H, opts_host, bw, fw, base + off, workspace_bytes - off, stream);
    if (rc) return rc;
    return fav_stream_next_frame_flows_lt(s, frame_rgb_hwc, m, bw, fw, use_structure, out_rgb_f32, out_rgb8_hwc, stream);
}
