// fav_stylize_vr -- drop-in for `th fast_artistic_video_vr.lua ...` (fast_artistic_video_vr.lua:21-76,561-591) on MI355X:
// stylises a 360-degree video given as six overlapping cube faces per frame.  Same single-dash flags, same file patterns
// (-input_pattern with two integers: frame, face id; flow / occlusion patterns with {..} = frame-1, [..] = frame and a
// remaining %d = face id, :105-115), faces processed in the order of ids {6,1,2,5,3,4} (:103), outputs
// "<prefix>-%05d_equi.png" / "<prefix>-%05d_cubemap.png" (:541,552).  All compute goes through libfav's C ABI (fav_vr_*);
// there is no CPU backend.  Not provided (rejected with a message): -evaluate, -backward, -smooth_certainty and
// -continue_with > 1 (in the reference that option reloads per-face PNGs which func_save_image no longer writes, :521-523).
// -forward_flow_pattern <pat> (additive; same {..} / [..] / %d tokens as -flow_pattern, e.g. flow-%d/forward_{%d}_[%d].flo): the
// forward-backward consistency check runs on the GPU from the two flows (fav_vr_face_flow) and no certainty file is read;
// -occlusions_pattern is then not required, and if both are given the forward flow wins.  -structure <0|1> (default 1, as
// makeOptFlow_deepflow.sh:59 calls the checker) selects the checker's 4-argument mode on the face's frame.  At the first face of a
// frame the masks of the faces whose files are complete already are started ahead of the faces (fav_vr_prefetch_mask).
// -input_equi_pattern <pat> (additive; one integer: the frame) selects a second mode by its input: the video's equirectangular frames
// INSTEAD of face, flow and certainty files (naming any of -input_pattern, -flow_pattern, -forward_flow_pattern, -occlusions_pattern next
// to it is an error).  Every frame is turned into six faces of -cube_edge_length <n> (768) pixels with -overlap_pixel_w / _h of margin
// (fav_vr_equi_to_faces_rgb8, -supersample <1..4>, default 2; the reference script's pair is 768 / 128), both flows of all six faces are
// estimated in one batched call (fav_flow_pairs_rgb8_ex3; -flow_alpha, -flow_eps, -flow_grad, -flow_match, -flow_median, -flow_warps, -flow_iters as in fav_stylize, 0 = default) and the faces
// run as with -forward_flow_pattern.  One GPU.  (-estimate_flow is NOT a flag here: the flows follow from there being no face files.)
// Additive flags: -precision <fp32|bf16>, -warp_border <stn|cpu>, -poll_timeout <sec>, -poll_settle <sec> (host/fav_poll.h), -png_level <0..9>, -seed <n> (uniform-random fill), -timing <0|1>,
// and -- several 360-degree videos on several GPUs (BASELINE config 5; the faces of one frame depend on each other through the
// border priors, so the unit of sharding is the video) -- -streams <a,b,...> / -gpus <n> / -force_dist / -dry_run exactly as in
// fav_stylize (host/fav_launcher.h): %S in -input_pattern, -flow_pattern, -forward_flow_pattern, -occlusions_pattern and -output_prefix is the stream's
// name, stream s -> worker process s mod n, rank 0 parses the checkpoints and ncclBroadcast (RCCL) hands the packed blobs on.
#include <hip/hip_runtime.h>
#include <sys/stat.h>
#include <unistd.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <future>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../include/fav.h"
#include "fav_cli.h"
#include "fav_launcher.h"
#include "fav_poll.h"

namespace {

using favl::die; using favl::check; using favl::file_exists; using favl::mkdirs_for; using favl::fmt_int; using favl::flow_name; using favl::read_polled;
using Flags = favl::Flags; using Bools = std::map<std::string, bool>;
void hipc(hipError_t e, const char* what) { if (e != hipSuccess) die(std::string(what) + ": " + hipGetErrorString(e)); }
template <class T> fav::dev_ptr<T> dev_alloc(size_t bytes) { return favl::dev_alloc<T>(bytes, "hipMalloc"); }

struct VrDestroy { void operator()(fav_vr* p) const { fav_vr_destroy(p); } };
using vr_h = std::unique_ptr<fav_vr, VrDestroy>;

static const int proc_order[6] = {6, 1, 2, 5, 3, 4};                                                               // :103

// a finished input: there, not empty and not modified for -poll_settle seconds (what wait_for_file accepts at its first look)
bool ready_now(const std::string& path, double settle_s)
{
    struct stat st;
    return stat(path.c_str(), &st) == 0 && S_ISREG(st.st_mode) && st.st_size > 0 && favp::wall_age_seconds(st) >= settle_s;
}

vr_h vr_create(Flags& v, Bools& b, fav_net* vid, fav_net* img, int H, int W)
{
    auto I = [&](const char* k) { return atoi(v[k].c_str()); };
    fav_vr_opts o{};
    o.overlap_w = I("overlap_pixel_w"); o.overlap_h = I("overlap_pixel_h"); o.occlusions_min_filter = I("occlusions_min_filter");
    o.median_filter = I("median_filter"); o.fill_random = v["fill_occlusions"] == "uniform-random"; o.seed = (unsigned)I("seed");
    o.create_inconsistent = b["create_inconsistent"]; o.create_inconsistent_border = b["create_inconsistent_border"];
    o.out_equi_w = b["out_equi"] ? I("out_equi_w") : 0; o.out_equi_h = b["out_equi"] ? I("out_equi_h") : 0;
    o.border_mode = v["warp_border"] == "cpu" ? FAV_BORDER_CPU : FAV_BORDER_STN;
    fav_vr* vr = nullptr;
    check(fav_vr_create(vid, img, H, W, &o, &vr), "fav_vr_create");
    return vr_h(vr);
}

// A finished frame's way out of the device, the same in both input modes (:527-557): the equirectangular and / or cube-map image,
// -png_encoder gpu (default): as finished PNG files (fav_png_encode_rgb8); host: zlib on the writer thread, -png_level.  One frame is
// written in the background while the next one computes.
struct VrOutput {
    int ew = 0, eh = 0, cw = 0, ch = 0;
    bool gpu_png = false; int png_level = 1; std::string prefix;
    fav::dev_ptr<uint8_t> d_equi, d_cube, d_png_e, d_png_c; fav::dev_ptr<uint32_t> d_png_n; fav::dev_ptr<void> d_png_ws;
    size_t png_ws_bytes = 0, cap_e = 0, cap_c = 0;
    std::vector<uint8_t> h_equi, h_cube;
    std::future<void> writer;

    void setup(fav_vr* vr, Flags& v, Bools& b)
    {
        gpu_png = v["png_encoder"] == "gpu"; png_level = atoi(v["png_level"].c_str()); prefix = v["output_prefix"];
        check(fav_vr_output_sizes(vr, &ew, &eh, &cw, &ch, nullptr, nullptr), "fav_vr_output_sizes");
        if (b["out_cubemap"] && !cw) die("-out_cubemap needs square cropped faces");
        if (gpu_png && (ew > 9000 || (b["out_cubemap"] && cw > 9000))) die("-png_encoder gpu encodes rows of up to 9000 pixels; pass -png_encoder host for these output sizes");
        if (ew) { d_equi = dev_alloc<uint8_t>((size_t)ew * eh * 3); h_equi.resize((size_t)ew * eh * 3); }
        if (b["out_cubemap"]) { d_cube = dev_alloc<uint8_t>((size_t)cw * ch * 3); h_cube.resize((size_t)cw * ch * 3); }
        if (!gpu_png) return;
        if (d_equi) { cap_e = fav_png_capacity(ew, eh); d_png_e = dev_alloc<uint8_t>(cap_e); h_equi.resize(cap_e); png_ws_bytes = std::max(png_ws_bytes, fav_png_workspace_bytes(ew, eh)); }
        if (d_cube) { cap_c = fav_png_capacity(cw, ch); d_png_c = dev_alloc<uint8_t>(cap_c); h_cube.resize(cap_c); png_ws_bytes = std::max(png_ws_bytes, fav_png_workspace_bytes(cw, ch)); }
        d_png_n = dev_alloc<uint32_t>(16);
        hipc(hipMemset(d_png_n.get(), 0, 16), "hipMemset");      // (the size word of an output that is not asked for is read back too)
        if (png_ws_bytes) d_png_ws = dev_alloc<void>(png_ws_bytes);
    }
    void wait() { if (writer.valid()) writer.get(); }
    // the six faces of frame out_idx are through: assemble, encode, download, and write in the background
    void write_frame(fav_vr* vr, fav_net* vid, int out_idx, hipStream_t st)
    {
        wait();
        check(fav_vr_finish_frame(vr, d_equi.get(), d_cube.get(), st), "fav_vr_finish_frame");
        uint32_t png_n[2] = {0, 0};
        if (gpu_png) {
            if (d_equi) check(fav_png_encode_rgb8(d_equi.get(), ew, eh, d_png_e.get(), cap_e, d_png_n.get(), d_png_ws.get(), png_ws_bytes, st), "fav_png_encode_rgb8");
            if (d_cube) check(fav_png_encode_rgb8(d_cube.get(), cw, ch, d_png_c.get(), cap_c, d_png_n.get() + 1, d_png_ws.get(), png_ws_bytes, st), "fav_png_encode_rgb8");   // (same stream: the workspace is free again)
            hipc(hipMemcpyAsync(png_n, d_png_n.get(), 8, hipMemcpyDeviceToHost, st), "D2H");
            hipc(hipStreamSynchronize(st), "sync");
            if (png_n[0] > cap_e || png_n[1] > cap_c) die("fav_png_encode_rgb8 returned an impossible size");
            if (d_equi) hipc(hipMemcpyAsync(h_equi.data(), d_png_e.get(), png_n[0], hipMemcpyDeviceToHost, st), "D2H");
            if (d_cube) hipc(hipMemcpyAsync(h_cube.data(), d_png_c.get(), png_n[1], hipMemcpyDeviceToHost, st), "D2H");
        } else {
            if (d_equi) hipc(hipMemcpyAsync(h_equi.data(), d_equi.get(), h_equi.size(), hipMemcpyDeviceToHost, st), "D2H");
            if (d_cube) hipc(hipMemcpyAsync(h_cube.data(), d_cube.get(), h_cube.size(), hipMemcpyDeviceToHost, st), "D2H");
        }
        hipc(hipStreamSynchronize(st), "sync");
        check(fav_net_check(vid), "finishing a frame");
        std::vector<uint8_t> e = h_equi, cb = h_cube;
        if (gpu_png) { e.resize(d_equi ? png_n[0] : 0); cb.resize(d_cube ? png_n[1] : 0); }
        writer = std::async(std::launch::async, [e, cb, out_idx, prefix = prefix, gpu = gpu_png, lvl = png_level, ew = ew, eh = eh, cw = cw, ch = ch]() {
            auto put = [&](const char* kind, const std::vector<uint8_t>& bytes, int pw, int ph) {
                if (bytes.empty()) return;
                char name[4096];
                snprintf(name, sizeof name, "%s-%05d_%s.png", prefix.c_str(), out_idx, kind); mkdirs_for(name);
                if (gpu) {                                                       // the bytes ARE the file
                    FILE* f = fopen(name, "wb");
                    if (!f || fwrite(bytes.data(), 1, bytes.size(), f) != bytes.size() || fclose(f)) die(std::string("writing ") + name + " failed");
                } else if (fav_write_png_rgb8_host(name, bytes.data(), pw, ph, lvl)) die(std::string("writing ") + name + ": " + fav_last_error());
            };
            put("equi", e, ew, eh); put("cubemap", cb, cw, ch);
        });
    }
};

// the end of a video, in the order that matters: the last file, the library's state, the networks' verdict, and the queue -- which
// the library must not wait on before the next video's first forward.  The caller's buffers go after it, the queue drained.
double end_video(VrOutput& out, vr_h& vr, fav::queue_h& st, fav_net* vid, fav_net* img, bool timing, int frames_done, std::chrono::steady_clock::time_point t_all)
{
    out.wait();
    if (timing && frames_done) {
        const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_all).count();
        printf("%d frames (x6 faces) in %.3f s: %.2f frames/s\n", frames_done, s, frames_done / s);
    }
    vr.reset();
    check(fav_net_check(vid), "stylising the video");
    if (img) check(fav_net_check(img), "stylising the video (image model)");
    (void)fav_net_forget_stream(vid, st.get());
    st.reset();
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t_all).count();
}

// one 360-degree video: the loop of run_fast_neural_video with fast_artistic_video_vr.lua's callbacks (:103-302,454-591)
int run_video(Flags& v, Bools& b, fav_net* vid, fav_net* img, double* seconds_out)
{
    auto I = [&](const char* k) { return atoi(v[k].c_str()); };
    const bool timing = I("timing") != 0;
    fav::queue_h st_h = favl::queue_create("hipStreamCreate"); hipStream_t const st = st_h.get();
    int W = 0, H = 0;
    // -forward_flow_pattern: the check runs on the device; the six faces of a frame then have their own input buffers (a mask started
    // ahead of its face reads them until that face is through), otherwise set 0 serves every face
    const bool fused = !v["forward_flow_pattern"].empty(); const int use_structure = I("structure");
    const int nset = fused ? 6 : 1;
    fav::dev_ptr<uint8_t> d_frame6[6], d_cert; fav::dev_ptr<float> d_bw6[6], d_fw6[6]; bool loaded[6] = {};
    VrOutput out;
    vr_h vr;                                 // declared after the buffers its side stream reads: it goes first
    favp::Poll poll; poll.timeout_s = atof(v["poll_timeout"].c_str()); poll.settle_s = std::max(0.0, atof(v["poll_settle"].c_str()));
    const int start = I("start_frame"), total = I("num_frames") * 6;                                              // :571
    const auto t_all = std::chrono::steady_clock::now();
    int frames_done = 0;
    for (int i = 1; i <= total; ++i) {
        const int mode = (i - 1) % 6, file_idx = (i - 1) / 6 + start, face = proc_order[mode];                     // :155-156
        const std::string img_path = fmt_int(v["input_pattern"], file_idx, face);
        if (!file_exists(img_path)) break;                                                                          // :160
        const bool temporal = i >= 7 && !b["create_inconsistent"];
        const int set = fused ? mode : 0;
        if (fused && temporal && mode == 0) {
            // look-ahead: the faces of this frame whose three files are complete already go to the device now and their masks start on
            // the library's side stream; a face that is not ready yet (or does not read) is loaded in its turn, polled as ever
            std::vector<void*> held;
            for (int k = 0; k < 6; ++k) {
                loaded[k] = false;
                const std::string ip = fmt_int(v["input_pattern"], file_idx, proc_order[k]);
                const std::string bp = flow_name(v["flow_pattern"], file_idx - 1, file_idx, proc_order[k]);
                const std::string fp = flow_name(v["forward_flow_pattern"], file_idx - 1, file_idx, proc_order[k]);
                if (!ready_now(ip, poll.settle_s) || !ready_now(bp, poll.settle_s) || !ready_now(fp, poll.settle_s)) continue;
                uint8_t* r8 = nullptr; float *bf = nullptr, *ff = nullptr; int iw = 0, ih = 0, ic = 0, bw_ = 0, bh_ = 0, fw_ = 0, fh_ = 0;
                const bool ok = fav_read_pnm_host(ip.c_str(), &r8, &iw, &ih, &ic) == 0 && fav_read_flo_host(bp.c_str(), &bf, &bw_, &bh_) == 0 &&
                                fav_read_flo_host(fp.c_str(), &ff, &fw_, &fh_) == 0 && ic == 3 && iw == W && ih == H && bw_ == W && bh_ == H && fw_ == W && fh_ == H;
                held.push_back(r8); held.push_back(bf); held.push_back(ff);
                if (!ok) continue;                                               // (its own turn reports what is wrong with it)
                hipc(hipMemcpyAsync(d_frame6[k].get(), r8, (size_t)W * H * 3, hipMemcpyHostToDevice, st), "H2D frame");
                hipc(hipMemcpyAsync(d_bw6[k].get(), bf, (size_t)W * H * 8, hipMemcpyHostToDevice, st), "H2D flow");
                hipc(hipMemcpyAsync(d_fw6[k].get(), ff, (size_t)W * H * 8, hipMemcpyHostToDevice, st), "H2D forward flow");
                check(fav_vr_prefetch_mask(vr.get(), i + k, d_frame6[k].get(), d_bw6[k].get(), d_fw6[k].get(), use_structure, st), "fav_vr_prefetch_mask");
                loaded[k] = true;
            }
            hipc(hipStreamSynchronize(st), "sync");                              // the copies have left the host buffers
            for (void* hp : held) fav_free_host(hp);
        }
        const bool have = fused && temporal && loaded[mode];                     // this face's inputs are on the device already
        uint8_t* rgb = nullptr; int w = W, h = H, c = 3;
        if (!have) check(fav_read_pnm_host(img_path.c_str(), &rgb, &w, &h, &c), "reading the face image");
        if (c != 3) die(img_path + ": not a P6 image");
        if (!vr) {
            W = w; H = h;
            vr = vr_create(v, b, vid, img, H, W);
            out.setup(vr.get(), v, b);
            for (int k = 0; k < nset; ++k) {
                d_frame6[k] = dev_alloc<uint8_t>((size_t)W * H * 3);
                d_bw6[k] = dev_alloc<float>((size_t)W * H * 8);
                if (fused) d_fw6[k] = dev_alloc<float>((size_t)W * H * 8);
            }
            if (!fused) d_cert = dev_alloc<uint8_t>((size_t)W * H);
        } else if (w != W || h != H) die(img_path + ": face size changed");
        uint8_t* d_frame = d_frame6[set].get(); float* d_flow = d_bw6[set].get(); float* d_fwd = d_fw6[set].get();
        if (!have) hipc(hipMemcpyAsync(d_frame, rgb, (size_t)W * H * 3, hipMemcpyHostToDevice, st), "H2D frame");
        float* flo = nullptr; float* fwd = nullptr; uint8_t* cert = nullptr;
        if (temporal && !have) {                                                                                    // :225-229, :274-278
            const std::string fp = flow_name(v["flow_pattern"], file_idx - 1, file_idx, face);
            int cw_ = W, ch_ = H, cc = 1, fw = 0, fh = 0, gw = W, gh = H;
            if (fused) {                                                         // the forward flow is waited for like the backward flow
                const std::string gp = flow_name(v["forward_flow_pattern"], file_idx - 1, file_idx, face);
                read_polled(gp, poll, "reading the forward flow", [&] { return fav_read_flo_host(gp.c_str(), &fwd, &gw, &gh); });
            } else {
                const std::string cp = flow_name(v["occlusions_pattern"], file_idx - 1, file_idx, face);
                read_polled(cp, poll, "reading the certainty", [&] { return fav_read_pnm_host(cp.c_str(), &cert, &cw_, &ch_, &cc); });
            }
            read_polled(fp, poll, "reading the flow", [&] { return fav_read_flo_host(fp.c_str(), &flo, &fw, &fh); });
            if (cc != 1 || cw_ != W || ch_ != H || fw != W || fh != H || gw != W || gh != H) die("flow / certainty size does not match the face: " + fp);
            if (cert) hipc(hipMemcpyAsync(d_cert.get(), cert, (size_t)W * H, hipMemcpyHostToDevice, st), "H2D cert");
            if (fwd) hipc(hipMemcpyAsync(d_fwd, fwd, (size_t)W * H * 8, hipMemcpyHostToDevice, st), "H2D forward flow");
            hipc(hipMemcpyAsync(d_flow, flo, (size_t)W * H * 8, hipMemcpyHostToDevice, st), "H2D flow");
        }
        const auto t0 = std::chrono::steady_clock::now();
        if (fused) check(fav_vr_face_flow(vr.get(), i, d_frame, temporal ? d_flow : nullptr, temporal ? d_fwd : nullptr, use_structure, nullptr, st), "fav_vr_face_flow");
        else check(fav_vr_face(vr.get(), i, d_frame, temporal ? d_flow : nullptr, temporal ? d_cert.get() : nullptr, nullptr, st), "fav_vr_face");
        hipc(hipStreamSynchronize(st), "sync");
        // a stream-K hand-off that timed out: fail at THIS face, before any output derived from it is written (fav.h: the check
        // comes before a PNG is queued); the image model stylises the faces without a prior
        check(fav_net_check(vid), "stylising a face");
        if (img) check(fav_net_check(img), "stylising a face (image model)");
        if (timing) printf("Elapsed time for stylizing face %d of frame %d: %.4f\n", face, file_idx, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
        fav_free_host(rgb); fav_free_host(flo); fav_free_host(fwd); fav_free_host(cert);
        if (mode == 5) { out.write_frame(vr.get(), vid, (i - 1) / 6 + 1, st); ++frames_done; }                      // :517 (not offset by -start_frame)
    }
    *seconds_out = end_video(out, vr, st_h, vid, img, timing, frames_done, t_all);
    return frames_done;
}

// -input_equi_pattern: the same video from its equirectangular frames alone.  Per frame one PPM goes to the device, one launch makes the
// six faces (fav_vr_equi_to_faces_rgb8), one batched call estimates the twelve flows between the previous faces and these
// (fav_flow_pairs_rgb8), the six masks start on the library's side stream and the faces run through fav_vr_face_flow as in the file
// mode with -forward_flow_pattern; no face, flow or certainty file exists.  Everything is enqueued on one stream.
int run_video_equi(Flags& v, Bools& b, const fav_flow_opts_ex3& fo, fav_net* vid, fav_net* img, double* seconds_out)
{
    auto I = [&](const char* k) { return atoi(v[k].c_str()); };
    const bool timing = I("timing") != 0, inconsistent = b["create_inconsistent"];
    const int W = I("cube_edge_length"), H = W, use_structure = I("structure"), start = I("start_frame"), count = I("num_frames");
    fav::queue_h st_h = favl::queue_create("hipStreamCreate"); hipStream_t const st = st_h.get();
    // two sets of six faces (previous, current), the twelve flows, the estimator's workspace, the source frame
    fav::dev_ptr<uint8_t> faces_h[2][6], d_src; fav::dev_ptr<float> bw_h[6], fw_h[6]; fav::dev_ptr<void> d_flow_ws;
    uint8_t* d_faces[2][6] = {}; float* d_bw[6] = {}; float* d_fw[6] = {};      // what the library's calls take: arrays of plain pointers
    VrOutput out;
    vr_h vr = vr_create(v, b, vid, img, H, W);        // declared after the buffers its side stream reads: it goes first
    out.setup(vr.get(), v, b);
    const size_t face_bytes = (size_t)W * H * 3, flow_bytes = (size_t)W * H * 8;
    for (int k = 0; k < 6; ++k) {
        d_faces[0][k] = (faces_h[0][k] = dev_alloc<uint8_t>(face_bytes)).get();
        d_faces[1][k] = (faces_h[1][k] = dev_alloc<uint8_t>(face_bytes)).get();
        if (!inconsistent) { d_bw[k] = (bw_h[k] = dev_alloc<float>(flow_bytes)).get(); d_fw[k] = (fw_h[k] = dev_alloc<float>(flow_bytes)).get(); }
    }
    size_t flow_ws_bytes = 0;
    if (!inconsistent) {
        flow_ws_bytes = fav_flow_pairs_workspace_bytes_ex3(W, H, 6, &fo);
        if (!flow_ws_bytes) die(std::string("-input_equi_pattern: ") + fav_last_error());
        d_flow_ws = dev_alloc<void>(flow_ws_bytes);
    }
    int sw = 0, sh = 0;
    const auto t_all = std::chrono::steady_clock::now();
    int frames_done = 0;
    for (int n = 0; n < count; ++n) {
        const int file_idx = start + n, cur = n & 1, prev = cur ^ 1;
        const std::string path = fmt_int(v["input_equi_pattern"], file_idx);
        if (!file_exists(path)) break;
        uint8_t* rgb = nullptr; int w = 0, h = 0, c = 0;
        check(fav_read_pnm_host(path.c_str(), &rgb, &w, &h, &c), "reading the equirectangular frame");
        if (c != 3) die(path + ": not a P6 image");
        if (!d_src) { sw = w; sh = h; d_src = dev_alloc<uint8_t>((size_t)w * h * 3); }
        else if (w != sw || h != sh) die(path + ": frame size changed");
        hipc(hipMemcpyAsync(d_src.get(), rgb, (size_t)sw * sh * 3, hipMemcpyHostToDevice, st), "H2D frame");
        check(fav_vr_equi_to_faces_rgb8(d_src.get(), sw, sh, H, W, I("overlap_pixel_w"), I("overlap_pixel_h"), I("supersample"), d_faces[cur], nullptr, st), "fav_vr_equi_to_faces_rgb8");
        const bool temporal = n > 0 && !inconsistent;
        const int i0 = n * 6 + 1;                                              // the frame's first face, 1-based and frame-major
        if (temporal) {
            check(fav_flow_pairs_rgb8_ex3(d_faces[prev], d_faces[cur], 6, W, H, &fo, d_bw, d_fw, d_flow_ws.get(), flow_ws_bytes, st), "fav_flow_pairs_rgb8_ex3");
            for (int k = 0; k < 6; ++k) check(fav_vr_prefetch_mask(vr.get(), i0 + k, d_faces[cur][k], d_bw[k], d_fw[k], use_structure, st), "fav_vr_prefetch_mask");
        }
        hipc(hipStreamSynchronize(st), "sync");                                // the copy has left the host buffer
        fav_free_host(rgb);
        for (int k = 0; k < 6; ++k) {
            const auto t0 = std::chrono::steady_clock::now();
            check(fav_vr_face_flow(vr.get(), i0 + k, d_faces[cur][k], temporal ? d_bw[k] : nullptr, temporal ? d_fw[k] : nullptr, use_structure, nullptr, st), "fav_vr_face_flow");
            hipc(hipStreamSynchronize(st), "sync");
            check(fav_net_check(vid), "stylising a face");                       // before any output derived from the face is written
            if (img) check(fav_net_check(img), "stylising a face (image model)");
            if (timing) printf("Elapsed time for stylizing face %d of frame %d: %.4f\n", proc_order[k], file_idx, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
        }
        out.write_frame(vr.get(), vid, n + 1, st);                              // :517 (not offset by -start_frame)
        ++frames_done;
    }
    *seconds_out = end_video(out, vr, st_h, vid, img, timing, frames_done, t_all);
    return frames_done;
}

}  // namespace

int main(int argc, char** argv)
{
    std::map<std::string, std::string> v = {
        {"input_pattern", ""}, {"input_equi_pattern", ""}, {"cube_edge_length", "768"}, {"supersample", "2"},
        {"flow_pattern", ""}, {"occlusions_pattern", ""}, {"forward_flow_pattern", ""}, {"structure", "1"}, {"model_img", ""}, {"model_vid", ""},
        {"start_frame", "1"}, {"continue_with", "1"}, {"num_frames", "9999"}, {"occlusions_min_filter", "7"},
        {"fill_occlusions", "vgg-mean"}, {"overlap_pixel_w", "20"}, {"overlap_pixel_h", "20"}, {"output_prefix", "out"},
        {"out_equi_w", "768"}, {"out_equi_h", "768"}, {"median_filter", "3"}, {"gpu", "-1"}, {"backend", "cuda"}, {"use_cudnn", "1"},
        {"cudnn_benchmark", "0"}, {"evaluation_file", "evaluation.txt"}, {"flow_pattern_eval", ""}, {"occlusions_pattern_eval", ""},
        {"content_weights", "1.0"}, {"content_layers", "16"}, {"loss_network", "models/vgg16.t7"}, {"style_image", ""},
        {"style_image_size", "256"}, {"style_weights", "5.0"}, {"style_layers", "4,9,16,23"}, {"style_target_type", "gram"},
        {"warp_border", "stn"}, {"poll_timeout", "600"}, {"poll_settle", "1.0"}, {"png_level", "1"}, {"png_encoder", "gpu"}, {"seed", "1"}, {"timing", "0"}, {"precision", "fp32"},
        {"streams", ""}, {"gpus", "1"}, {"force_dist", "0"}, {"dry_run", "0"}, {"pin_workers", "1"}, {"worker_rank", "-1"}, {"worker_world", "0"}, {"rccl_id_file", ""}};
    std::map<std::string, bool> b = {
        {"invert_occlusions", false}, {"fix_occlusions", false}, {"smooth_certainty", false}, {"create_inconsistent", false},
        {"create_inconsistent_border", false}, {"backward", false}, {"out_equi", false}, {"out_cubemap", false}, {"evaluate", false},
        {"no_consistency_eval", false}, {"invert_occlusions_eval", false}, {"backward_eval", false}, {"fix_occlusions_eval", false}};
    favl::add_flow_flags(v);
    for (int a = 1; a < argc; ++a) {                       // torch.CmdLine: -flag value | -boolflag
        std::string k = argv[a];
        if (k.size() < 2 || k[0] != '-') die("unknown argument " + k);
        k = k.substr(1);
        if (b.count(k)) { b[k] = true; continue; }
        if (!v.count(k)) die("unknown option -" + k);
        if (a + 1 >= argc) die("missing value for -" + k);
        v[k] = argv[++a];
    }
    auto I = [&](const char* k) { return atoi(v[k].c_str()); };
    // -input_equi_pattern: the faces are made from the equirectangular frames and both flows of every face are estimated from them, so
    // no face, flow or certainty file exists and none may be named
    const bool from_equi = !v["input_equi_pattern"].empty();
    favl::validate_flow_flags(v, from_equi, "-input_equi_pattern");
    const fav_flow_opts_ex3 fo = favl::flow_opts_of(v);      // used by run_video_equi
    if (from_equi) {
        for (const char* k : {"input_pattern", "flow_pattern", "forward_flow_pattern", "occlusions_pattern"})
            if (!v[k].empty()) die(std::string("-input_equi_pattern makes the faces and their flows from the equirectangular frames: it cannot be combined with -") + k);
        if (I("supersample") < 1 || I("supersample") > 4) die("-supersample must be 1 .. 4, not '" + v["supersample"] + "'");
        if (I("cube_edge_length") < 16 || I("cube_edge_length") > 16384) die("-cube_edge_length must be 16 .. 16384, not '" + v["cube_edge_length"] + "'");
        if (fav_flow_workspace_bytes_ex3(64, 64, &fo) == 0) die(std::string("-flow_alpha / -flow_eps / -flow_iters / -flow_warps: ") + fav_last_error());
        if (std::max(1, I("gpus")) > 1 || I("force_dist")) die("-input_equi_pattern runs on one GPU: it cannot be combined with -gpus > 1 or -force_dist");
    }
    if (!from_equi && v["input_pattern"].empty()) die("Must give -input_pattern");                                  // :564-566
    // (-forward_flow_pattern: the certainty is computed from the two flows, -occlusions_pattern is not needed -- and not read if given)
    if (!from_equi && !b["create_inconsistent"] && (v["flow_pattern"].empty() || (v["occlusions_pattern"].empty() && v["forward_flow_pattern"].empty())))
        die("Must give -flow_pattern and -occlusions_pattern");                                                     // :567-569
    if (v["structure"] != "0" && v["structure"] != "1") die("-structure must be 0 or 1");
    if (!v["forward_flow_pattern"].empty() && !v["occlusions_pattern"].empty() && atoi(v["worker_rank"].c_str()) < 0)
        fprintf(stderr, "fav_stylize_vr: -forward_flow_pattern and -occlusions_pattern both given: the forward flow wins (the check runs on the GPU, no certainty file is read)\n");
    if (I("gpu") < 0) die("-gpu -1: this build has no CPU backend (the CPU restatement under oracle/ is test infrastructure); pass -gpu <id>");
    if (b["evaluate"]) die("-evaluate (perceptual / edge losses) is outside the hot-path scope");
    if (b["backward"]) die("-backward is not provided for the cube-map pipeline");
    if (b["smooth_certainty"]) die("-smooth_certainty is not provided");
    if (I("continue_with") != 1) die("-continue_with > 1 reloads per-face PNGs that the reference no longer writes (fast_artistic_video_vr.lua:521-523); not provided");
    if (v["model_vid"].empty()) die("Must give -model_vid");
    if (v["fill_occlusions"] != "vgg-mean" && v["fill_occlusions"] != "uniform-random") die("-fill_occlusions must be vgg-mean or uniform-random");
    if (v["precision"] != "fp32" && v["precision"] != "bf16") die("-precision must be fp32 or bf16");
    if (v["png_encoder"] != "gpu" && v["png_encoder"] != "host") die("-png_encoder must be gpu or host");
    const bool timing = I("timing") != 0, dry = I("dry_run") != 0;
    std::vector<std::string> streams = favl::split_list(v["streams"]);
    const bool named = !streams.empty();
    if (!named) streams.push_back("");
    int world = std::max(1, I("gpus"));
    const int rank = I("worker_rank");
    static const char* const path_opts[] = {"input_pattern", "input_equi_pattern", "flow_pattern", "occlusions_pattern", "forward_flow_pattern", "output_prefix"};
    if (named && streams.size() > 1 && v["output_prefix"].find("%S") == std::string::npos)
        die("-streams: -output_prefix must contain %S (the videos would overwrite each other's frames)");
    if (rank < 0 && (world > 1 || I("force_dist"))) {                                   // launcher: one worker process per GPU
        if (!dry) {
            std::vector<std::string> models{v["model_vid"]};
            if (!v["model_img"].empty() && v["model_img"] != "self") models.push_back(v["model_img"]);
            favl::validate_models(models);                        // before any worker exists
            const int ndev = fav_device_count();
            if (ndev <= 0) die(std::string("ERROR: ") + fav_last_error());
            if (I("gpu") + world > ndev) die("-gpus " + v["gpus"] + " from -gpu " + v["gpu"] + ": only " + std::to_string(ndev) + " devices");
        }
        std::string xdir;
        const int worst = favl::spawn_workers(argc, argv, world, I("pin_workers") != 0, &xdir);
        if (timing && !dry && worst == 0) favl::print_aggregate(xdir, world, streams.size());
        favl::remove_exchange_dir(xdir, world);
        return worst;
    }
    const bool dist = rank >= 0;
    if (dist) world = I("worker_world");
    const int device = I("gpu") + (dist ? rank : 0);
    std::vector<std::string> mine;
    for (size_t s_ = 0; s_ < streams.size(); ++s_) if (!dist || (int)(s_ % (size_t)world) == rank) mine.push_back(streams[s_]);
    if (dry) {
        favl::dry_run_failure_hook(rank);
        std::string js = "{\"rank\": " + std::to_string(std::max(rank, 0)) + ", \"world\": " + std::to_string(dist ? world : 1) + ", \"device\": " + std::to_string(device) + ", \"streams\": [";
        for (size_t k = 0; k < mine.size(); ++k) {
            js += std::string(k ? ", " : "") + "{\"name\": " + favl::json_str(mine[k]);
            for (const char* po : path_opts) js += std::string(", \"") + po + "\": " + favl::json_str(named ? favl::subst_stream(v[po], mine[k]) : v[po]);
            js += "}";
        }
        printf("%s]}\n", js.c_str());
        return 0;
    }

    hipc(hipSetDevice(device), "hipSetDevice");
    fav_net* vid = nullptr; fav_net* img = nullptr;
    const bool want_img = !v["model_img"].empty() && v["model_img"] != "self";
    if (dist) {
        favl::load_models_dist(rank, world, v["rccl_id_file"], device, v["model_vid"], want_img ? v["model_img"] : std::string(), &vid, &img, mine.size(), 1);
    } else {
        if (fav_net_create(v["model_vid"].c_str(), device, &vid)) die(std::string("ERROR: Could not load model from ") + v["model_vid"] + " (" + fav_last_error() + ")");
        if (want_img && fav_net_create(v["model_img"].c_str(), device, &img)) die(std::string("ERROR: Could not load model from ") + v["model_img"] + " (" + fav_last_error() + ")");
    }
    check(fav_net_set_precision(vid, v["precision"] == "bf16" ? FAV_PRECISION_BF16_OPERANDS : FAV_PRECISION_FP32), "fav_net_set_precision");
    int frames = 0; double seconds = 0;
    for (const std::string& name : mine) {
        std::map<std::string, std::string> vs = v;
        if (named) for (const char* po : path_opts) vs[po] = favl::subst_stream(v[po], name);
        double sec = 0;
        frames += from_equi ? run_video_equi(vs, b, fo, vid, img, &sec) : run_video(vs, b, vid, img, &sec);
        seconds += sec;
    }
    if (dist && timing) favl::write_worker_result(v["rccl_id_file"], rank, frames, seconds);
    if (img) fav_net_destroy(img);
    fav_net_destroy(vid);
    return 0;
}
