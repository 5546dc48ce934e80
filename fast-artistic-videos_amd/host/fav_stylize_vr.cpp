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
#include <string>
#include <vector>

#include "../../include/fav.h"
#include "fav_launcher.h"
#include "fav_poll.h"

namespace {

using favl::die;
void check(int rc, const char* what) { if (rc) die(std::string(what) + ": " + fav_last_error()); }
void hipc(hipError_t e, const char* what) { if (e != hipSuccess) die(std::string(what) + ": " + hipGetErrorString(e)); }
bool file_exists(const std::string& p) { struct stat st; return stat(p.c_str(), &st) == 0 && S_ISREG(st.st_mode); }

std::string fmt1(const std::string& pattern, int a) { char b[4096]; snprintf(b, sizeof b, pattern.c_str(), a); return b; }
std::string fmt2(const std::string& pattern, int a, int c) { char b[4096]; snprintf(b, sizeof b, pattern.c_str(), a, c); return b; }

// getFormatedFlowFileName (fast_artistic_video_vr.lua:105-115): {fmt} <- from, [fmt] <- to, then the remaining %d <- face id
std::string flow_name(const std::string& pattern, int from, int to, int face)
{
    std::string out;
    for (size_t p = 0; p < pattern.size();) {
        const char c = pattern[p];
        if (c == '{' || c == '[') {
            const size_t e = pattern.find(c == '{' ? '}' : ']', p + 1);
            if (e != std::string::npos) { out += fmt1(pattern.substr(p + 1, e - p - 1), c == '{' ? from : to); p = e + 1; continue; }
        }
        out += c; ++p;
    }
    return fmt1(out, face);
}

// utils.lua:74-80 with the settle rule of fav_poll.h: wait, read, poll again while the file reads short under its producer
template <class Reader>
void read_polled(const std::string& path, const favp::Poll& p, const char* what, Reader&& reader)
{
    bool timed_out = false;
    const int rc = favp::read_when_complete(path, p, reader, &timed_out);
    if (timed_out) die("timed out waiting for " + path);
    check(rc, what);
}

// a finished input: there, not empty and not modified for -poll_settle seconds (what wait_for_file accepts at its first look)
bool ready_now(const std::string& path, double settle_s)
{
    struct stat st;
    return stat(path.c_str(), &st) == 0 && S_ISREG(st.st_mode) && st.st_size > 0 && favp::wall_age_seconds(st) >= settle_s;
}

void mkdirs_for(const std::string& path)
{
    for (size_t p = 1; p < path.size(); ++p) if (path[p] == '/') mkdir(path.substr(0, p).c_str(), 0777);
}

// one 360-degree video: the loop of run_fast_neural_video with fast_artistic_video_vr.lua's callbacks (:103-302,454-591)
int run_video(std::map<std::string, std::string>& v, std::map<std::string, bool>& b, fav_net* vid, fav_net* img, double* seconds_out)
{
    auto I = [&](const char* k) { return atoi(v[k].c_str()); };
    const bool timing = I("timing") != 0;
    static const int proc_order[6] = {6, 1, 2, 5, 3, 4};                                                           // :103
    hipStream_t st; hipc(hipStreamCreate(&st), "hipStreamCreate");
    fav_vr* vr = nullptr;
    int W = 0, H = 0, ew = 0, eh = 0, cw = 0, ch = 0;
    // -forward_flow_pattern: the check runs on the device; the six faces of a frame then have their own input buffers (a mask started
    // ahead of its face reads them until that face is through), otherwise set 0 serves every face
    const bool fused = !v["forward_flow_pattern"].empty(); const int use_structure = I("structure");
    const int nset = fused ? 6 : 1;
    uint8_t* d_frame6[6] = {}; float* d_bw6[6] = {}; float* d_fw6[6] = {}; bool loaded[6] = {};
    uint8_t *d_cert = nullptr, *d_equi = nullptr, *d_cube = nullptr;
    favp::Poll poll; poll.timeout_s = atof(v["poll_timeout"].c_str()); poll.settle_s = std::max(0.0, atof(v["poll_settle"].c_str()));
    std::vector<uint8_t> h_equi, h_cube;
    // -png_encoder gpu (default): the two output images leave the device as finished PNG files (fav_png_encode_rgb8); host: zlib, -png_level
    const bool gpu_png = v["png_encoder"] == "gpu";
    uint8_t *d_png_e = nullptr, *d_png_c = nullptr; uint32_t* d_png_n = nullptr; void* d_png_ws = nullptr; size_t png_ws_bytes = 0, cap_e = 0, cap_c = 0;
    std::future<void> writer;
    const int start = I("start_frame"), total = I("num_frames") * 6;                                              // :571
    const auto t_all = std::chrono::steady_clock::now();
    int frames_done = 0;
    for (int i = 1; i <= total; ++i) {
        const int mode = (i - 1) % 6, file_idx = (i - 1) / 6 + start, face = proc_order[mode];                     // :155-156
        const std::string img_path = fmt2(v["input_pattern"], file_idx, face);
        if (!file_exists(img_path)) break;                                                                          // :160
        const bool temporal = i >= 7 && !b["create_inconsistent"];
        const int set = fused ? mode : 0;
        if (fused && temporal && mode == 0) {
            // look-ahead: the faces of this frame whose three files are complete already go to the device now and their masks start on
            // the library's side stream; a face that is not ready yet (or does not read) is loaded in its turn, polled as ever
            std::vector<void*> held;
            for (int k = 0; k < 6; ++k) {
                loaded[k] = false;
                const std::string ip = fmt2(v["input_pattern"], file_idx, proc_order[k]);
                const std::string bp = flow_name(v["flow_pattern"], file_idx - 1, file_idx, proc_order[k]);
                const std::string fp = flow_name(v["forward_flow_pattern"], file_idx - 1, file_idx, proc_order[k]);
                if (!ready_now(ip, poll.settle_s) || !ready_now(bp, poll.settle_s) || !ready_now(fp, poll.settle_s)) continue;
                uint8_t* r8 = nullptr; float *bf = nullptr, *ff = nullptr; int iw = 0, ih = 0, ic = 0, bw_ = 0, bh_ = 0, fw_ = 0, fh_ = 0;
                const bool ok = fav_read_pnm_host(ip.c_str(), &r8, &iw, &ih, &ic) == 0 && fav_read_flo_host(bp.c_str(), &bf, &bw_, &bh_) == 0 &&
                                fav_read_flo_host(fp.c_str(), &ff, &fw_, &fh_) == 0 && ic == 3 && iw == W && ih == H && bw_ == W && bh_ == H && fw_ == W && fh_ == H;
                held.push_back(r8); held.push_back(bf); held.push_back(ff);
                if (!ok) continue;                                               // (its own turn reports what is wrong with it)
                hipc(hipMemcpyAsync(d_frame6[k], r8, (size_t)W * H * 3, hipMemcpyHostToDevice, st), "H2D frame");
                hipc(hipMemcpyAsync(d_bw6[k], bf, (size_t)W * H * 8, hipMemcpyHostToDevice, st), "H2D flow");
                hipc(hipMemcpyAsync(d_fw6[k], ff, (size_t)W * H * 8, hipMemcpyHostToDevice, st), "H2D forward flow");
                check(fav_vr_prefetch_mask(vr, i + k, d_frame6[k], d_bw6[k], d_fw6[k], use_structure, st), "fav_vr_prefetch_mask");
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
            fav_vr_opts o{};
            o.overlap_w = I("overlap_pixel_w"); o.overlap_h = I("overlap_pixel_h"); o.occlusions_min_filter = I("occlusions_min_filter");
            o.median_filter = I("median_filter"); o.fill_random = v["fill_occlusions"] == "uniform-random"; o.seed = (unsigned)I("seed");
            o.create_inconsistent = b["create_inconsistent"]; o.create_inconsistent_border = b["create_inconsistent_border"];
            o.out_equi_w = b["out_equi"] ? I("out_equi_w") : 0; o.out_equi_h = b["out_equi"] ? I("out_equi_h") : 0;
            o.border_mode = v["warp_border"] == "cpu" ? FAV_BORDER_CPU : FAV_BORDER_STN;
            check(fav_vr_create(vid, img, H, W, &o, &vr), "fav_vr_create");
            check(fav_vr_output_sizes(vr, &ew, &eh, &cw, &ch, nullptr, nullptr), "fav_vr_output_sizes");
            if (b["out_cubemap"] && !cw) die("-out_cubemap needs square cropped faces");
            for (int k = 0; k < nset; ++k) {
                hipc(hipMalloc(reinterpret_cast<void**>(&d_frame6[k]), (size_t)W * H * 3), "hipMalloc");
                hipc(hipMalloc(reinterpret_cast<void**>(&d_bw6[k]), (size_t)W * H * 8), "hipMalloc");
                if (fused) hipc(hipMalloc(reinterpret_cast<void**>(&d_fw6[k]), (size_t)W * H * 8), "hipMalloc");
            }
            if (!fused) hipc(hipMalloc(reinterpret_cast<void**>(&d_cert), (size_t)W * H), "hipMalloc");
            if (ew) { hipc(hipMalloc(reinterpret_cast<void**>(&d_equi), (size_t)ew * eh * 3), "hipMalloc"); h_equi.resize((size_t)ew * eh * 3); }
            if (b["out_cubemap"]) { hipc(hipMalloc(reinterpret_cast<void**>(&d_cube), (size_t)cw * ch * 3), "hipMalloc"); h_cube.resize((size_t)cw * ch * 3); }
            if (gpu_png && (ew > 9000 || (b["out_cubemap"] && cw > 9000))) die("-png_encoder gpu encodes rows of up to 9000 pixels; pass -png_encoder host for these output sizes");
            if (gpu_png) {
                if (ew) { cap_e = fav_png_capacity(ew, eh); hipc(hipMalloc(reinterpret_cast<void**>(&d_png_e), cap_e), "hipMalloc"); h_equi.resize(cap_e); png_ws_bytes = std::max(png_ws_bytes, fav_png_workspace_bytes(ew, eh)); }
                if (b["out_cubemap"]) { cap_c = fav_png_capacity(cw, ch); hipc(hipMalloc(reinterpret_cast<void**>(&d_png_c), cap_c), "hipMalloc"); h_cube.resize(cap_c); png_ws_bytes = std::max(png_ws_bytes, fav_png_workspace_bytes(cw, ch)); }
                hipc(hipMalloc(reinterpret_cast<void**>(&d_png_n), 16), "hipMalloc");
                hipc(hipMemset(d_png_n, 0, 16), "hipMemset");      // (the size word of an output that is not asked for is read back too)
                if (png_ws_bytes) hipc(hipMalloc(&d_png_ws, png_ws_bytes), "hipMalloc");
            }
        } else if (w != W || h != H) die(img_path + ": face size changed");
        uint8_t* d_frame = d_frame6[set]; float* d_flow = d_bw6[set]; float* d_fwd = d_fw6[set];
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
            if (cert) hipc(hipMemcpyAsync(d_cert, cert, (size_t)W * H, hipMemcpyHostToDevice, st), "H2D cert");
            if (fwd) hipc(hipMemcpyAsync(d_fwd, fwd, (size_t)W * H * 8, hipMemcpyHostToDevice, st), "H2D forward flow");
            hipc(hipMemcpyAsync(d_flow, flo, (size_t)W * H * 8, hipMemcpyHostToDevice, st), "H2D flow");
        }
        const auto t0 = std::chrono::steady_clock::now();
        if (fused) check(fav_vr_face_flow(vr, i, d_frame, temporal ? d_flow : nullptr, temporal ? d_fwd : nullptr, use_structure, nullptr, st), "fav_vr_face_flow");
        else check(fav_vr_face(vr, i, d_frame, temporal ? d_flow : nullptr, temporal ? d_cert : nullptr, nullptr, st), "fav_vr_face");
        hipc(hipStreamSynchronize(st), "sync");
        // a stream-K hand-off that timed out: fail at THIS face, before any output derived from it is written (fav.h: the check
        // comes before a PNG is queued); the image model stylises the faces without a prior
        check(fav_net_check(vid), "stylising a face");
        if (img) check(fav_net_check(img), "stylising a face (image model)");
        if (timing) printf("Elapsed time for stylizing face %d of frame %d: %.4f\n", face, file_idx, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
        fav_free_host(rgb); fav_free_host(flo); fav_free_host(fwd); fav_free_host(cert);
        if (mode == 5) {                                                                                            // :527-557
            if (writer.valid()) writer.get();
            check(fav_vr_finish_frame(vr, d_equi, b["out_cubemap"] ? d_cube : nullptr, st), "fav_vr_finish_frame");
            uint32_t png_n[2] = {0, 0};
            if (gpu_png) {
                if (d_equi) check(fav_png_encode_rgb8(d_equi, ew, eh, d_png_e, cap_e, d_png_n, d_png_ws, png_ws_bytes, st), "fav_png_encode_rgb8");
                if (d_cube) check(fav_png_encode_rgb8(d_cube, cw, ch, d_png_c, cap_c, d_png_n + 1, d_png_ws, png_ws_bytes, st), "fav_png_encode_rgb8");   // (same stream: the workspace is free again)
                hipc(hipMemcpyAsync(png_n, d_png_n, 8, hipMemcpyDeviceToHost, st), "D2H");
                hipc(hipStreamSynchronize(st), "sync");
                if (png_n[0] > cap_e || png_n[1] > cap_c) die("fav_png_encode_rgb8 returned an impossible size");
                if (d_equi) hipc(hipMemcpyAsync(h_equi.data(), d_png_e, png_n[0], hipMemcpyDeviceToHost, st), "D2H");
                if (d_cube) hipc(hipMemcpyAsync(h_cube.data(), d_png_c, png_n[1], hipMemcpyDeviceToHost, st), "D2H");
            } else {
                if (d_equi) hipc(hipMemcpyAsync(h_equi.data(), d_equi, h_equi.size(), hipMemcpyDeviceToHost, st), "D2H");
                if (d_cube) hipc(hipMemcpyAsync(h_cube.data(), d_cube, h_cube.size(), hipMemcpyDeviceToHost, st), "D2H");
            }
            hipc(hipStreamSynchronize(st), "sync");
            check(fav_net_check(vid), "finishing a frame");
            const int out_idx = (i - 1) / 6 + 1;                                                                    // :517 (not offset by -start_frame)
            const std::string prefix = v["output_prefix"]; const int lvl = I("png_level");
            std::vector<uint8_t> e = h_equi, cb = h_cube;
            if (gpu_png) { e.resize(d_equi ? png_n[0] : 0); cb.resize(d_cube ? png_n[1] : 0); }
            writer = std::async(std::launch::async, [=]() {
                char name[4096];
                auto put = [&](const char* nm, const std::vector<uint8_t>& bytes) {          // the bytes ARE the file (GPU encoder)
                    FILE* f = fopen(nm, "wb");
                    if (!f || fwrite(bytes.data(), 1, bytes.size(), f) != bytes.size() || fclose(f)) die(std::string("writing ") + nm + " failed");
                };
                if (!e.empty()) {
                    snprintf(name, sizeof name, "%s-%05d_equi.png", prefix.c_str(), out_idx); mkdirs_for(name);
                    if (gpu_png) put(name, e);
                    else if (fav_write_png_rgb8_host(name, e.data(), ew, eh, lvl)) die(std::string("writing ") + name + ": " + fav_last_error());
                }
                if (!cb.empty()) {
                    snprintf(name, sizeof name, "%s-%05d_cubemap.png", prefix.c_str(), out_idx); mkdirs_for(name);
                    if (gpu_png) put(name, cb);
                    else if (fav_write_png_rgb8_host(name, cb.data(), cw, ch, lvl)) die(std::string("writing ") + name + ": " + fav_last_error());
                }
            });
            ++frames_done;
        }
    }
    if (writer.valid()) writer.get();
    if (timing && frames_done) {
        const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_all).count();
        printf("%d frames (x6 faces) in %.3f s: %.2f frames/s\n", frames_done, s, frames_done / s);
    }
    if (vr) fav_vr_destroy(vr);
    check(fav_net_check(vid), "stylising the video");
    if (img) check(fav_net_check(img), "stylising the video (image model)");
    for (int k = 0; k < 6; ++k) { (void)hipFree(d_frame6[k]); (void)hipFree(d_bw6[k]); (void)hipFree(d_fw6[k]); }
    (void)hipFree(d_cert); (void)hipFree(d_equi); (void)hipFree(d_cube);
    (void)hipFree(d_png_e); (void)hipFree(d_png_c); (void)hipFree(d_png_n); (void)hipFree(d_png_ws);
    (void)fav_net_forget_stream(vid, st);      // the library must not wait on this handle before the next video's first forward
    hipStreamDestroy(st);
    *seconds_out = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_all).count();
    return frames_done;
}

// -input_equi_pattern: the same video from its equirectangular frames alone.  Per frame one PPM goes to the device, one launch makes the
// six faces (fav_vr_equi_to_faces_rgb8), one batched call estimates the twelve flows between the previous faces and these
// (fav_flow_pairs_rgb8), the six masks start on the library's side stream and the faces run through fav_vr_face_flow as in the file
// mode with -forward_flow_pattern; no face, flow or certainty file exists.  Everything is enqueued on one stream.  (run_video above is
// the reference's file contract and stays as it is; the frame's way out of the device is restated here.)
int run_video_equi(std::map<std::string, std::string>& v, std::map<std::string, bool>& b, const fav_flow_opts_ex3& fo, fav_net* vid, fav_net* img, double* seconds_out)
{
    auto I = [&](const char* k) { return atoi(v[k].c_str()); };
    const bool timing = I("timing") != 0, gpu_png = v["png_encoder"] == "gpu", inconsistent = b["create_inconsistent"];
    static const int proc_order[6] = {6, 1, 2, 5, 3, 4};                                                           // :103
    const int W = I("cube_edge_length"), H = W, use_structure = I("structure"), start = I("start_frame"), count = I("num_frames");
    hipStream_t st; hipc(hipStreamCreate(&st), "hipStreamCreate");
    fav_vr* vr = nullptr;
    fav_vr_opts o{};
    o.overlap_w = I("overlap_pixel_w"); o.overlap_h = I("overlap_pixel_h"); o.occlusions_min_filter = I("occlusions_min_filter");
    o.median_filter = I("median_filter"); o.fill_random = v["fill_occlusions"] == "uniform-random"; o.seed = (unsigned)I("seed");
    o.create_inconsistent = inconsistent; o.create_inconsistent_border = b["create_inconsistent_border"];
    o.out_equi_w = b["out_equi"] ? I("out_equi_w") : 0; o.out_equi_h = b["out_equi"] ? I("out_equi_h") : 0;
    o.border_mode = v["warp_border"] == "cpu" ? FAV_BORDER_CPU : FAV_BORDER_STN;
    check(fav_vr_create(vid, img, H, W, &o, &vr), "fav_vr_create");
    int ew = 0, eh = 0, cw = 0, ch = 0;
    check(fav_vr_output_sizes(vr, &ew, &eh, &cw, &ch, nullptr, nullptr), "fav_vr_output_sizes");
    if (b["out_cubemap"] && !cw) die("-out_cubemap needs square cropped faces");
    if (gpu_png && (ew > 9000 || (b["out_cubemap"] && cw > 9000))) die("-png_encoder gpu encodes rows of up to 9000 pixels; pass -png_encoder host for these output sizes");
    // two sets of six faces (previous, current), the twelve flows, the estimator's workspace, the source frame
    const size_t face_bytes = (size_t)W * H * 3, flow_bytes = (size_t)W * H * 8;
    uint8_t* d_faces[2][6] = {}; float* d_bw[6] = {}; float* d_fw[6] = {};
    for (int k = 0; k < 6; ++k) {
        hipc(hipMalloc(reinterpret_cast<void**>(&d_faces[0][k]), face_bytes), "hipMalloc");
        hipc(hipMalloc(reinterpret_cast<void**>(&d_faces[1][k]), face_bytes), "hipMalloc");
        if (!inconsistent) { hipc(hipMalloc(reinterpret_cast<void**>(&d_bw[k]), flow_bytes), "hipMalloc"); hipc(hipMalloc(reinterpret_cast<void**>(&d_fw[k]), flow_bytes), "hipMalloc"); }
    }
    void* d_flow_ws = nullptr; size_t flow_ws_bytes = 0;
    if (!inconsistent) {
        flow_ws_bytes = fav_flow_pairs_workspace_bytes_ex3(W, H, 6, &fo);
        if (!flow_ws_bytes) die(std::string("-input_equi_pattern: ") + fav_last_error());
        hipc(hipMalloc(&d_flow_ws, flow_ws_bytes), "hipMalloc");
    }
    uint8_t *d_src = nullptr, *d_equi = nullptr, *d_cube = nullptr; int sw = 0, sh = 0;
    std::vector<uint8_t> h_equi, h_cube;
    uint8_t *d_png_e = nullptr, *d_png_c = nullptr; uint32_t* d_png_n = nullptr; void* d_png_ws = nullptr; size_t png_ws_bytes = 0, cap_e = 0, cap_c = 0;
    if (ew) { hipc(hipMalloc(reinterpret_cast<void**>(&d_equi), (size_t)ew * eh * 3), "hipMalloc"); h_equi.resize((size_t)ew * eh * 3); }
    if (b["out_cubemap"]) { hipc(hipMalloc(reinterpret_cast<void**>(&d_cube), (size_t)cw * ch * 3), "hipMalloc"); h_cube.resize((size_t)cw * ch * 3); }
    if (gpu_png) {
        if (ew) { cap_e = fav_png_capacity(ew, eh); hipc(hipMalloc(reinterpret_cast<void**>(&d_png_e), cap_e), "hipMalloc"); h_equi.resize(cap_e); png_ws_bytes = std::max(png_ws_bytes, fav_png_workspace_bytes(ew, eh)); }
        if (b["out_cubemap"]) { cap_c = fav_png_capacity(cw, ch); hipc(hipMalloc(reinterpret_cast<void**>(&d_png_c), cap_c), "hipMalloc"); h_cube.resize(cap_c); png_ws_bytes = std::max(png_ws_bytes, fav_png_workspace_bytes(cw, ch)); }
        hipc(hipMalloc(reinterpret_cast<void**>(&d_png_n), 16), "hipMalloc");
        hipc(hipMemset(d_png_n, 0, 16), "hipMemset");
        if (png_ws_bytes) hipc(hipMalloc(&d_png_ws, png_ws_bytes), "hipMalloc");
    }
    std::future<void> writer;
    const auto t_all = std::chrono::steady_clock::now();
    int frames_done = 0;
    for (int n = 0; n < count; ++n) {
        const int file_idx = start + n, cur = n & 1, prev = cur ^ 1;
        const std::string path = fmt1(v["input_equi_pattern"], file_idx);
        if (!file_exists(path)) break;
        uint8_t* rgb = nullptr; int w = 0, h = 0, c = 0;
        check(fav_read_pnm_host(path.c_str(), &rgb, &w, &h, &c), "reading the equirectangular frame");
        if (c != 3) die(path + ": not a P6 image");
        if (!d_src) { sw = w; sh = h; hipc(hipMalloc(reinterpret_cast<void**>(&d_src), (size_t)w * h * 3), "hipMalloc"); }
        else if (w != sw || h != sh) die(path + ": frame size changed");
        hipc(hipMemcpyAsync(d_src, rgb, (size_t)sw * sh * 3, hipMemcpyHostToDevice, st), "H2D frame");
        check(fav_vr_equi_to_faces_rgb8(d_src, sw, sh, H, W, o.overlap_w, o.overlap_h, I("supersample"), d_faces[cur], nullptr, st), "fav_vr_equi_to_faces_rgb8");
        const bool temporal = n > 0 && !inconsistent;
        const int i0 = n * 6 + 1;                                              // the frame's first face, 1-based and frame-major
        if (temporal) {
            check(fav_flow_pairs_rgb8_ex3(d_faces[prev], d_faces[cur], 6, W, H, &fo, d_bw, d_fw, d_flow_ws, flow_ws_bytes, st), "fav_flow_pairs_rgb8_ex3");
            for (int k = 0; k < 6; ++k) check(fav_vr_prefetch_mask(vr, i0 + k, d_faces[cur][k], d_bw[k], d_fw[k], use_structure, st), "fav_vr_prefetch_mask");
        }
        hipc(hipStreamSynchronize(st), "sync");                                // the copy has left the host buffer
        fav_free_host(rgb);
        for (int k = 0; k < 6; ++k) {
            const auto t0 = std::chrono::steady_clock::now();
            check(fav_vr_face_flow(vr, i0 + k, d_faces[cur][k], temporal ? d_bw[k] : nullptr, temporal ? d_fw[k] : nullptr, use_structure, nullptr, st), "fav_vr_face_flow");
            hipc(hipStreamSynchronize(st), "sync");
            check(fav_net_check(vid), "stylising a face");                       // before any output derived from the face is written
            if (img) check(fav_net_check(img), "stylising a face (image model)");
            if (timing) printf("Elapsed time for stylizing face %d of frame %d: %.4f\n", proc_order[k], file_idx, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
        }
        if (writer.valid()) writer.get();
        check(fav_vr_finish_frame(vr, d_equi, d_cube, st), "fav_vr_finish_frame");
        uint32_t png_n[2] = {0, 0};
        if (gpu_png) {
            if (d_equi) check(fav_png_encode_rgb8(d_equi, ew, eh, d_png_e, cap_e, d_png_n, d_png_ws, png_ws_bytes, st), "fav_png_encode_rgb8");
            if (d_cube) check(fav_png_encode_rgb8(d_cube, cw, ch, d_png_c, cap_c, d_png_n + 1, d_png_ws, png_ws_bytes, st), "fav_png_encode_rgb8");
            hipc(hipMemcpyAsync(png_n, d_png_n, 8, hipMemcpyDeviceToHost, st), "D2H");
            hipc(hipStreamSynchronize(st), "sync");
            if (png_n[0] > cap_e || png_n[1] > cap_c) die("fav_png_encode_rgb8 returned an impossible size");
            if (d_equi) hipc(hipMemcpyAsync(h_equi.data(), d_png_e, png_n[0], hipMemcpyDeviceToHost, st), "D2H");
            if (d_cube) hipc(hipMemcpyAsync(h_cube.data(), d_png_c, png_n[1], hipMemcpyDeviceToHost, st), "D2H");
        } else {
            if (d_equi) hipc(hipMemcpyAsync(h_equi.data(), d_equi, h_equi.size(), hipMemcpyDeviceToHost, st), "D2H");
            if (d_cube) hipc(hipMemcpyAsync(h_cube.data(), d_cube, h_cube.size(), hipMemcpyDeviceToHost, st), "D2H");
        }
        hipc(hipStreamSynchronize(st), "sync");
        check(fav_net_check(vid), "finishing a frame");
        const int out_idx = n + 1;                                              // :517 (not offset by -start_frame)
        const std::string prefix = v["output_prefix"]; const int lvl = I("png_level");
        std::vector<uint8_t> e = h_equi, cb = h_cube;
        if (gpu_png) { e.resize(d_equi ? png_n[0] : 0); cb.resize(d_cube ? png_n[1] : 0); }
        writer = std::async(std::launch::async, [=]() {
            auto put = [&](const char* kind, const std::vector<uint8_t>& bytes, int pw, int ph) {
                if (bytes.empty()) return;
                char name[4096];
                snprintf(name, sizeof name, "%s-%05d_%s.png", prefix.c_str(), out_idx, kind); mkdirs_for(name);
                if (gpu_png) {                                                   // the bytes ARE the file
                    FILE* f = fopen(name, "wb");
                    if (!f || fwrite(bytes.data(), 1, bytes.size(), f) != bytes.size() || fclose(f)) die(std::string("writing ") + name + " failed");
                } else if (fav_write_png_rgb8_host(name, bytes.data(), pw, ph, lvl)) die(std::string("writing ") + name + ": " + fav_last_error());
            };
            put("equi", e, ew, eh); put("cubemap", cb, cw, ch);
        });
        ++frames_done;
    }
    if (writer.valid()) writer.get();
    if (timing && frames_done) {
        const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_all).count();
        printf("%d frames (x6 faces) in %.3f s: %.2f frames/s\n", frames_done, s, frames_done / s);
    }
    fav_vr_destroy(vr);
    check(fav_net_check(vid), "stylising the video");
    if (img) check(fav_net_check(img), "stylising the video (image model)");
    for (int k = 0; k < 6; ++k) { (void)hipFree(d_faces[0][k]); (void)hipFree(d_faces[1][k]); (void)hipFree(d_bw[k]); (void)hipFree(d_fw[k]); }
    (void)hipFree(d_flow_ws); (void)hipFree(d_src); (void)hipFree(d_equi); (void)hipFree(d_cube);
    (void)hipFree(d_png_e); (void)hipFree(d_png_c); (void)hipFree(d_png_n); (void)hipFree(d_png_ws);
    (void)fav_net_forget_stream(vid, st);
    hipStreamDestroy(st);
    *seconds_out = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_all).count();
    return frames_done;
}

}  // namespace

int main(int argc, char** argv)
{
    std::map<std::string, std::string> v = {
        {"input_pattern", ""}, {"input_equi_pattern", ""}, {"cube_edge_length", "768"}, {"supersample", "2"}, {"flow_alpha", "0"}, {"flow_eps", "0"}, {"flow_grad", "0"}, {"flow_match", "0"}, {"flow_median", "0"}, {"flow_warps", "0"}, {"flow_iters", "0"},
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
    if (v["flow_grad"] != "0" && v["flow_grad"] != "1") die("-flow_grad must be 0 or 1, not '" + v["flow_grad"] + "'");
    if (I("flow_grad") && !from_equi) die("-flow_grad 1 selects the data term of the built-in flow estimator: it needs -input_equi_pattern");
    // the estimator's options from the -flow_* flags: validated here, used by run_video_equi
    if (v["flow_match"] != "0" && v["flow_match"] != "1") die("-flow_match must be 0 or 1, not '" + v["flow_match"] + "'");
    if (I("flow_match") && !from_equi) die("-flow_match 1 turns on the matching prior of the built-in flow estimator: it needs -input_equi_pattern");
    if (v["flow_median"] != "0" && v["flow_median"] != "3" && v["flow_median"] != "5") die("-flow_median must be 0, 3 or 5, not '" + v["flow_median"] + "'");
    if (I("flow_median") && !from_equi) die("-flow_median " + v["flow_median"] + " turns on the median filter of the built-in flow estimator: it needs -input_equi_pattern");
    const fav_flow_opts_ex3 fo{{{{0, I("flow_warps"), I("flow_iters"), (float)atof(v["flow_alpha"].c_str()), 0, (float)atof(v["flow_eps"].c_str())}, I("flow_grad")},
                                I("flow_match") ? -1.f : 0.f, 0},
                               I("flow_median")};
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
