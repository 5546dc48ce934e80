// fav_stylize -- drop-in for `th fast_artistic_video.lua ...` (fast_artistic_video.lua:21-67,174-189 +
// fast_artistic_video_core.lua:34-229) on MI355X.  Same single-dash flags, same file-name patterns
// ({..} = index i-1, [..] = index i; fast_artistic_video.lua:70-77), same 1-based frame loop that stops
// at the first missing frame (core.lua:196-197), same "<prefix>-%05d.png" outputs (fav.lua:161).
//
// Host structure: loader threads read/decode frames i+1.. (PPM, .flo, .pgm) into pinned staging while the GPU works on
// frame i; uploads run on their own queue; the host enqueues frame i before it waits for frame i-1 (so the GPU never idles
// between frames); PNG deflate + file writes run on a small pool.  All compute
// goes through libfav's C ABI (fav_stream_*); there is no CPU backend (-gpu -1 is rejected).
//
// Additive flags (not in the reference): -forward_flow_pattern <pat> (run the consistency check on the
// GPU instead of reading .pgm files), -structure <0|1> (4-argument checker mode, default 1 as in
// makeOptFlow_deepflow.sh:59), -warp_border <stn|cpu>, -poll_timeout <sec>, -poll_settle <sec> (1.0: a file younger than this is
//   taken only once it has not been modified for that long -- what utils.lua:79's `sleep 1` buys; host/fav_poll.h),
// -png_overlap <0|1> (0, default; 1: with -png_encoder gpu the encoder's kernels run on a queue of their own next to the following frame's
//   network -- fav_stream_encode_png_async -- instead of in front of it: +0.5 % in HBM, but the events between the queues cost this
//   process 1.6 ms of CPU per frame and the file -> PNG rate does not move, profiles/bench_r5e.log against bench_r5f.log)
// -png_encoder <gpu|host> (gpu, default: the PNG file's bytes are produced on the device, the host only write()s them -- fixed-Huffman
// deflate, larger files; host: zlib on the writer threads at -png_level <0..9>, ~25 ms per 1280x720 frame and core),
// -precision <fp32|bf16> (fp32 = parity mode, default; bf16 = optional fast mode, see include/fav.h),
// -seed <n> (key of the documented RNG behind -fill_occlusions uniform-random, unseeded in the reference),
// -writers <n>, -timing <0|1>, -temporal_eval_file <path> (the temporal-consistency number of -evaluate, fav.lua:128-151,
// with the frame's own flow and certainty: one line of ';'-separated per-frame values, one line with their mean),
// -estimate_flow <0|1> (0, default; 1: frames in, stylised PNGs out, no .flo / .pgm on disk -- both flows of a frame are estimated on the
//   device from frame i and the frame before it in processing order, which stays on the device (fav_stream_next_frame_estimate), and go
//   through the fused consistency check, -structure as usual.  Needs -input_pattern only; -flow_pattern, -forward_flow_pattern and
//   -occlusions_pattern are refused next to it, and so is a -scale_factor other than 1.  -continue_with reads frame i-1's file as well.
//   The 4-argument look-ahead is OFF in this mode: a mask needs the flows, and those do not exist before the frame is enqueued),
// -flow_alpha <x>, -flow_iters <n>, -flow_warps <n>, -flow_levels <n> (fav_flow_opts; 0 = default, each); -flow_eps <x> (smooth_eps: the
// edge-preserving smoothness, 0 = off, the default); -flow_grad <0|1> (fav_flow_opts_ex.data_term: the data term on the image gradients
// instead of the grey levels, for video whose lighting changes; 0 = off, the default; only with -estimate_flow 1); -flow_match <0|1>
// (fav_flow_opts_ex2.match_beta: the block-matching prior for objects that move further than their own size; 0 = off, the default; only
// with -estimate_flow 1); -flow_median <0|3|5> (fav_flow_opts_ex3.median: median filtering of the flow after every warp, the side of the
// window; 0 = off, the default; only with -estimate_flow 1).
// -input_y4m <path|-> INSTEAD of -input_pattern: the frames are those of a YUV4MPEG2 stream (`ffmpeg ... -f yuv4mpegpipe -`), frame i is
//   its i-th frame (1-based), read sequentially (a pipe's short reads included); the planes are uploaded and converted on the device
//   (fav_yuv_to_rgb8) into the buffer the PPM payload otherwise fills.  The stream ending at a frame boundary ends the clip like a missing
//   next file; ending INSIDE a frame is an error that names the frame, after the complete frames before it have been written.
// -output_y4m <path|-> INSTEAD of PNG files (-output_prefix and -png_* are unused): the input's header with the stylised frames' size
//   (without -input_y4m: F25:1 Ip A1:1), then per frame `FRAME` and the planes the device wrote into pinned memory
//   (fav_stream_encode_yuv), in order.  With `-` every message goes to stderr: stdout carries the stream and nothing else.
// -y4m_matrix <auto|bt601|bt709>, -y4m_range <auto|limited|full>: override what the input's header says or lacks (auto: XCOLORRANGE,
//   else limited; BT.709 from 720 rows on, else BT.601 -- Y4M carries no matrix); -y4m_format <420jpeg|420mpeg2|444>: the output's
//   sampling when it is not to be the input's (without -input_y4m the default is 420jpeg).
//   -y4m_pixel_format <tag> sets the output's whole layout instead, by Y4M's own C value: 420jpeg, 420mpeg2, 422, 444, and 420pN, 422pN,
//   444pN with N in 9, 10, 12, 14, 16 (include/fav_yuv.h).  The input may be any of these: a 10-bit 4:2:2 video in is a 10-bit 4:2:2 video
//   out.  Above 8 bits the stylised frame's floats reach the samples unquantised.  Not both of -y4m_format and -y4m_pixel_format.
//   Refused: -backward with -input_y4m, -continue_with other than 1 with either, `-` with more than one -streams entry.
// -scene_cut <T> (0, default: off; T in (0, 1]; only with -estimate_flow 1): restart the recurrence at scene changes.  Frame i, in
//   processing order, is a CUT when score(frame i-1, frame i) > T, the score being fav_scene_change_rgb8's block-histogram distance
//   total / (2 W H) in [0, 1] (include/fav.h).  A cut frame takes the path of a frame without a prior (fav_stream_first_frame: the image
//   model when -model_img names one, no flow estimated, 0 in -temporal_eval_file); the frame after it continues from its result.  The
//   measure is enqueued behind the upload of frame i, one frame ahead, into host-mapped memory: the host reads it a frame later and never
//   waits for a network.  Dissolves and fades are not detected; a flash is a cut.  Refused: without -estimate_flow 1, with
//   -create_inconsistent, a value outside [0, 1].
// -scene_cut_log <path> (only with -scene_cut): one line per frame, `index total score cut` (cut = 0 | 1; the first frame is
//   `index 0 0 0`), written when the frame is decided.
// -long_term <d[,d...]> (empty, default: off; only with -estimate_flow 1): LONG-TERM PRIORS.  The list names the distances beyond 1,
//   ascending, each in 2..16, at most three: -long_term 2,4 warps the stylised frames i-1, i-2 and i-4 to frame i, and every pixel takes
//   the nearest of them in which it was visible (Ruder et al. 2016, section 4.2; include/fav_long_term.h, DESIGN.md "Long-term priors"): what a
//   moving object uncovers continues from before it was covered.  The frames and stylised frames further back live in the library's
//   history (fav_stream_set_long_term); each distance costs one more pair of flows per frame, estimated in the same batched call, and the
//   -flow_* flags, the certainty options and -structure apply to every distance alike.  A frame without a prior (the first one, a
//   -scene_cut) restarts the history: frame i after a restart at r uses the distances d <= i - r.  -temporal_eval_file keeps measuring
//   distance 1.  Refused: without -estimate_flow 1 (flows from files exist for distance 1 only), with -create_inconsistent, a malformed list.
// -original_colors <0|1> (0, default): 1 keeps the INPUT frame's colours and takes only the luminance of the stylised frame (Gatys et al.,
//   "Preserving color in neural artistic style transfer"; the arithmetic is in include/fav.h and DESIGN.md, "Original colours").  Only what
//   leaves through the sink changes: the state that is warped into the next frame stays the network's full-colour output, and
//   -temporal_eval_file keeps measuring that state.  The matrix of the luminance is the output format's with -output_y4m, else BT.709 from
//   720 rows on and BT.601 below; -y4m_matrix bt601|bt709 overrides either.  Works through all three sinks (-png_encoder gpu | host,
//   -output_y4m); with -png_encoder gpu the encode is the synchronous one whatever -png_overlap says.  Refused with a Y4M output that is
//   4:2:2 or deeper than 8 bits: the colour transfer writes 8-bit 4:2:0 / 4:4:4 planes only.
//   Refused: a value other than 0 / 1; -continue_with above 1 (it reloads the previous PNG as the recurrent state, and with this flag the
//   PNG is not the state); at the first frame, stylised frames whose size is not the input's (sizes that are no multiples of 4).
//   fav_stylize_vr and the `th` shim do not take the flag.
//
// Several videos on several GPUs (BASELINE config 4; the reference runs one `th` process per video, stylizeVideo_deepflow.sh:87-96,
// and its only device hook is utils.setup_gpu, fast_artistic_video/utils.lua:43-66):
//   -streams <a,b,c,...>  independent videos; every path option (-input_pattern, -flow_pattern, -forward_flow_pattern,
//                         -occlusions_pattern, -output_prefix, -temporal_eval_file) has the token %S replaced by the stream's name
//   -gpus <n>             one worker PROCESS per GPU (devices -gpu .. -gpu+n-1), stream s -> worker s mod n, streams of a worker run
//                         back to back.  Rank 0 parses the checkpoint(s) once and broadcasts the packed blob (fav_net_pack_host) with
//                         RCCL (ncclBroadcast over xGMI; ncclCommInitRank + a unique-id file); no other collective: a stream's
//                         frame i needs its own frame i-1 only.  Each worker gets host-threads / n PNG writers and loaders.
//   -shared_gpu 1         the GPU is shared with other processes: data-parallel convolution grids (fav_net_set_shared_device)
//   -force_dist 1         take the worker / RCCL path even for -gpus 1;  -dry_run 1: workers print their assignment and exit
//                         without touching a device (plumbing test).
#include <hip/hip_runtime.h>
#include <dirent.h>
#include <fcntl.h>
#include <sys/resource.h>
#include <time.h>
#include <sys/stat.h>
#include <sys/wait.h>
#include <unistd.h>
#include <zlib.h>

#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <future>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/fav.h"
#include "fav_cli.h"
#include "fav_launcher.h"
#include "fav_poll.h"
#include "fav_y4m.h"

namespace {

struct Opt {
    std::map<std::string, std::string> v;
    std::map<std::string, bool> b;
    std::string s(const char* k) const { return v.at(k); }
    int i(const char* k) const { return atoi(v.at(k).c_str()); }
    double d(const char* k) const { return atof(v.at(k).c_str()); }
    bool f(const char* k) const { return b.at(k); }
};

using favl::die; using favl::check; using favl::file_exists; using favl::mkdirs_for; using favl::fmt_int; using favl::flow_name;

// diagnostic switches exist in -DFAV_DIAG builds of this executable only (csrc/fav_internal.h says why)
const char* diag_env(const char* name)
{
#ifdef FAV_DIAG
    return getenv(name);
#else
    (void)name;
    return nullptr;
#endif
}

// a polled read whose failure names the file
template <class Reader>
void read_polled(const std::string& path, const favp::Poll& p, Reader&& reader) { favl::read_polled(path, p, path.c_str(), reader); }

// minimal PNG reader for -continue_with (8-bit RGB / RGBA / grey, non-interlaced)
bool read_png_rgb8(const std::string& path, std::vector<uint8_t>& rgb, int& W, int& H)
{
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return false;
    std::vector<uint8_t> d;
    uint8_t buf[65536]; size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) d.insert(d.end(), buf, buf + got);
    fclose(f);
    if (d.size() < 33 || memcmp(d.data(), "\x89PNG\r\n\x1a\n", 8)) return false;
    auto be32 = [&](size_t p) { return (uint32_t)d[p] << 24 | (uint32_t)d[p + 1] << 16 | (uint32_t)d[p + 2] << 8 | d[p + 3]; };
    size_t p = 8; int ctype = -1, depth = 0, interlace = 0; std::vector<uint8_t> idat;
    while (p + 12 <= d.size()) {
        const uint32_t len = be32(p); const char* ty = (const char*)&d[p + 4];
        if (p + 12 + len > d.size()) return false;
        if (!memcmp(ty, "IHDR", 4)) { W = (int)be32(p + 8); H = (int)be32(p + 12); depth = d[p + 16]; ctype = d[p + 17]; interlace = d[p + 20]; }
        else if (!memcmp(ty, "IDAT", 4)) idat.insert(idat.end(), d.begin() + p + 8, d.begin() + p + 8 + len);
        else if (!memcmp(ty, "IEND", 4)) break;
        p += 12 + len;
    }
    const int ch = ctype == 2 ? 3 : ctype == 6 ? 4 : ctype == 0 ? 1 : 0;
    if (!ch || depth != 8 || interlace || W <= 0 || H <= 0) return false;
    const size_t stride = (size_t)W * ch;
    std::vector<uint8_t> raw((stride + 1) * H);
    uLongf rl = (uLongf)raw.size();
    if (uncompress(raw.data(), &rl, idat.data(), (uLong)idat.size()) != Z_OK || rl != raw.size()) return false;
    std::vector<uint8_t> img(stride * H);
    for (int y = 0; y < H; ++y) {
        const uint8_t ft = raw[(stride + 1) * y];
        const uint8_t* s = &raw[(stride + 1) * y + 1];
        uint8_t* o = &img[stride * y];
        const uint8_t* up = y ? &img[stride * (y - 1)] : nullptr;
        for (size_t x = 0; x < stride; ++x) {
            const int a = x >= (size_t)ch ? o[x - ch] : 0, b = up ? up[x] : 0, c = (up && x >= (size_t)ch) ? up[x - ch] : 0;
            int pr = 0;
            if (ft == 1) pr = a; else if (ft == 2) pr = b; else if (ft == 3) pr = (a + b) / 2;
            else if (ft == 4) { const int pp = a + b - c, pa = abs(pp - a), pb = abs(pp - b), pc = abs(pp - c); pr = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c); }
            o[x] = (uint8_t)(s[x] + pr);
        }
    }
    rgb.resize((size_t)W * H * 3);
    for (size_t i = 0; i < (size_t)W * H; ++i)
        for (int c = 0; c < 3; ++c) rgb[i * 3 + c] = img[i * ch + (ch == 1 ? 0 : c)];
    return true;
}

// tiny thread pool for PNG encode + write
class Pool {
public:
    explicit Pool(int n, int device = -1) { for (int i = 0; i < n; ++i) th_.emplace_back([this, device] { if (device >= 0) (void)hipSetDevice(device); run(); }); }
    ~Pool() { { std::lock_guard<std::mutex> l(m_); stop_ = true; } cv_.notify_all(); for (auto& t : th_) t.join(); }
    void submit(std::function<void()> f) { { std::lock_guard<std::mutex> l(m_); q_.push_back(std::move(f)); ++pending_; } cv_.notify_one(); }
    void wait_below(size_t n) { std::unique_lock<std::mutex> l(m_); done_.wait(l, [&] { return pending_ <= n; }); }
private:
    void run()
    {
        for (;;) {
            std::function<void()> f;
            { std::unique_lock<std::mutex> l(m_); cv_.wait(l, [&] { return stop_ || !q_.empty(); }); if (q_.empty()) return; f = std::move(q_.front()); q_.pop_front(); }
            f();
            { std::lock_guard<std::mutex> l(m_); --pending_; }
            done_.notify_all();
        }
    }
    std::vector<std::thread> th_; std::deque<std::function<void()>> q_; std::mutex m_; std::condition_variable cv_, done_;
    size_t pending_ = 0; bool stop_ = false;
};

// Pinned PNG output slots with explicit ownership: a slot is taken before the D2H copy of a frame is enqueued and released by
// the writer task once the file is on disk.  (Counting pending tasks is not enough: tasks finish out of order, so the oldest
// slot -- the next one a round-robin hands out -- may still be read by its writer.)
class Slots {
public:
    void add(uint8_t* p) { std::lock_guard<std::mutex> l(m_); free_.push_back(p); }
    uint8_t* take() { std::unique_lock<std::mutex> l(m_); cv_.wait(l, [&] { return !free_.empty(); }); uint8_t* p = free_.back(); free_.pop_back(); return p; }
    uint8_t* try_take() { std::lock_guard<std::mutex> l(m_); if (free_.empty()) return nullptr; uint8_t* p = free_.back(); free_.pop_back(); return p; }
    void give(uint8_t* p) { { std::lock_guard<std::mutex> l(m_); free_.push_back(p); } cv_.notify_one(); }
private:
    std::mutex m_; std::condition_variable cv_; std::vector<uint8_t*> free_;
};

struct FrameIn {           // everything frame i needs from disk
    int index = 0; bool ok = false; bool single = false;
    uint8_t* frame = nullptr; int W = 0, H = 0;
    float* bw = nullptr; float* fw = nullptr; uint8_t* cert = nullptr;
    uint8_t* yuv = nullptr;          // -input_y4m: the frame's planes instead of `frame`
    void release() { fav_free_host(frame); fav_free_host(bw); fav_free_host(fw); fav_free_host(cert); free(yuv); frame = yuv = nullptr; bw = fw = nullptr; cert = nullptr; }
};


struct StreamResult { int frames = 0; double seconds = 0, wait_loader = 0, wait_gpu = 0, wait_png = 0, setup = 0, tail = 0, cpu_s = 0, cpu_loaders = 0, cpu_writers = 0, cpu_writer_sync = 0, cpu_main = 0; long long png_bytes = 0; };

// Waiting for an event WITHOUT occupying a core: hipEventSynchronize spins on this runtime even for events created with
// hipEventBlockingSync (measured: 1.8 ms of CPU per 1.8 ms frame in the thread that waits, profiles/r03g_e2e.log), so the host polls
// with short sleeps instead.  The host runs a frame ahead of the GPU, so the added latency (<= the sleep) is never on the GPU's path.
hipError_t wait_event_sleeping(hipEvent_t ev, unsigned sleep_us = 100)
{
    for (;;) {
        const hipError_t e = hipEventQuery(ev);
        if (e != hipErrorNotReady) return e;
        usleep(sleep_us);
    }
}

double thread_cpu_seconds()
{
    struct timespec ts;
    if (clock_gettime(CLOCK_THREAD_CPUTIME_ID, &ts)) return 0.0;
    return ts.tv_sec + 1e-9 * ts.tv_nsec;
}

// CPU time of every live thread of the process (name: seconds), for -timing: the HIP runtime's own threads show up here
std::string thread_cpu_report()
{
    std::string out = "[";
    DIR* d = opendir("/proc/self/task");
    if (!d) return "[]";
    const double tick = 1.0 / (double)sysconf(_SC_CLK_TCK);
    bool first = true;
    while (struct dirent* e = readdir(d)) {
        if (e->d_name[0] == '.') continue;
        const std::string p = std::string("/proc/self/task/") + e->d_name + "/stat";
        FILE* f = fopen(p.c_str(), "r");
        if (!f) continue;
        char buf[1024]; const size_t n = fread(buf, 1, sizeof buf - 1, f); fclose(f); buf[n] = 0;
        const char* lp = strchr(buf, '('); const char* rp = strrchr(buf, ')');
        if (!lp || !rp) continue;
        std::string comm(lp + 1, rp);
        unsigned long ut = 0, stt = 0; char state;
        // fields after ')': state ppid pgrp session tty tpgid flags minflt cminflt majflt cmajflt utime stime
        if (sscanf(rp + 2, "%c %*d %*d %*d %*d %*d %*u %*u %*u %*u %*u %lu %lu", &state, &ut, &stt) != 3) continue;
        const double sec = (ut + stt) * tick;
        if (sec < 0.02) continue;
        char item[128]; snprintf(item, sizeof item, "%s{\"thread\": \"%s\", \"cpu_s\": %.2f}", first ? "" : ", ", comm.c_str(), sec);
        out += item; first = false;
    }
    closedir(d);
    return out + "]";
}

double process_cpu_seconds()
{
    struct rusage ru;
    if (getrusage(RUSAGE_SELF, &ru)) return 0.0;
    return ru.ru_utime.tv_sec + ru.ru_stime.tv_sec + 1e-6 * (ru.ru_utime.tv_usec + ru.ru_stime.tv_usec);
}

// one pinned staging set of the loader pipeline: what frame i's files decode into
struct Pinned { fav::host_ptr<uint8_t> frame, cert, yuv; fav::host_ptr<float> bw, fw; };

// Everything frame i needs from disk (fast_artistic_video.lua:93-110,153-158): the frame, and for a frame with a predecessor the backward
// flow plus either the certainty file (the reference's path: polled, fav.lua:102) or the forward flow (fused check).
// pd != null: decode straight into that pinned staging set of pin_px pixels (no allocation, no second copy)
// y4m != null (-input_y4m): the frame is the stream's i-th, W x H its header's size, y4m_bytes a frame's payload
FrameIn load_frame_inputs(const Opt& o, const favp::Poll& poll, int i, bool first_of_run, const Pinned* pd, size_t pin_px,
                          favy::Reader* y4m = nullptr, size_t y4m_bytes = 0)
{
    const bool estimate = o.i("estimate_flow") != 0;
    const bool fused_check = !o.s("forward_flow_pattern").empty();
    FrameIn in; in.index = pd ? -i - 1 : i;              // negative index marks "pinned, do not free"
    if (y4m) {
        in.yuv = pd ? pd->yuv.get() : static_cast<uint8_t*>(malloc(y4m_bytes));
        if (!in.yuv) die("out of host memory");
        // anything but a complete frame ends the clip here; the frame loop reports a stream that ended inside a frame once the frames
        // before it are written
        if (y4m->read_frame(i, in.yuv) != favy::Reader::FRAME) { if (!pd) { free(in.yuv); in.yuv = nullptr; } return in; }
        in.W = y4m->header().W; in.H = y4m->header().H;
    } else {
        const std::string fp = fmt_int(o.s("input_pattern"), i);
        if (!file_exists(fp)) return in;                                                                 // fav.lua:93-97 -> nil -> break
        int ch;
        if (pd) { check(fav_read_pnm_into_host(fp.c_str(), pd->frame.get(), pin_px * 3, &in.W, &in.H, &ch), fp.c_str()); in.frame = pd->frame.get(); }
        else check(fav_read_pnm_host(fp.c_str(), &in.frame, &in.W, &in.H, &ch), fp.c_str());
        if (ch != 3) die(fp + ": expected a colour (P6) frame");
    }
    in.single = (i == 1) || o.f("create_inconsistent") || first_of_run;                                 // fav.lua:172
    if (!in.single && !estimate) {
        const std::string fl = flow_name(o.s("flow_pattern"), i - 1, i);                               // fav.lua:100,154
        int w, h;
        if (fused_check) {
            const std::string ff = flow_name(o.s("forward_flow_pattern"), i - 1, i);
            read_polled(ff, poll, [&] { if (pd) { in.fw = pd->fw.get(); return fav_read_flo_into_host(ff.c_str(), in.fw, pin_px * 2, &w, &h); }
                                        return fav_read_flo_host(ff.c_str(), &in.fw, &w, &h); });
            if (w != in.W || h != in.H) die(ff + ": size differs from the frame");
        } else {
            const std::string cp = flow_name(o.s("occlusions_pattern"), i - 1, i);
            int cch = 0;
            read_polled(cp, poll, [&] { if (pd) { in.cert = pd->cert.get(); return fav_read_pnm_into_host(cp.c_str(), in.cert, pin_px, &w, &h, &cch); }   // fav.lua:102
                                        return fav_read_pnm_host(cp.c_str(), &in.cert, &w, &h, &cch); });
            if (cch != 1 || w != in.W || h != in.H) die(cp + ": expected a P5 mask of the frame's size");
        }
        read_polled(fl, poll, [&] { if (pd) { in.bw = pd->bw.get(); return fav_read_flo_into_host(fl.c_str(), in.bw, pin_px * 2, &w, &h); }
                                    return fav_read_flo_host(fl.c_str(), &in.bw, &w, &h); });
        if (w != in.W || h != in.H) die(fl + ": size differs from the frame");
    }
    in.ok = true;
    return in;
}

// The format of a Y4M stream's frames.  from_header: what the input's header says (null: there is no Y4M input -- 4:2:0 with centre
// siting, limited range, BT.709 from 720 rows on, else BT.601: the heuristic players use, Y4M carries no matrix); -y4m_matrix and
// -y4m_range override either; -y4m_format sets the OUTPUT's sampling, -y4m_pixel_format its sampling, siting and depth.  main has
// validated the four options.
bool y4m_pixel_format_layout(const std::string& tag, fav_yuv_layout* out);
fav_yuv_layout y4m_layout_of(const Opt& o, const fav_yuv_layout* from_header, int H, bool output)
{
    fav_yuv_layout f = from_header ? *from_header
                                   : fav_yuv_layout{(uint32_t)sizeof(fav_yuv_layout), FAV_YUV_420, FAV_YUV_SITING_CENTER, H >= 720 ? FAV_YUV_BT709 : FAV_YUV_BT601, 0, 8};
    if (o.s("y4m_matrix") != "auto") f.matrix = o.s("y4m_matrix") == "bt709" ? FAV_YUV_BT709 : FAV_YUV_BT601;
    if (o.s("y4m_range") != "auto") f.full_range = o.s("y4m_range") == "full";
    if (output && !o.s("y4m_format").empty()) {
        f.chroma = o.s("y4m_format") == "444" ? FAV_YUV_444 : FAV_YUV_420;
        f.siting = o.s("y4m_format") == "420mpeg2" ? FAV_YUV_SITING_LEFT : FAV_YUV_SITING_CENTER;
        f.depth = 8;
    }
    if (output && !o.s("y4m_pixel_format").empty()) {
        fav_yuv_layout t;
        y4m_pixel_format_layout(o.s("y4m_pixel_format"), &t);
        f.chroma = t.chroma; f.siting = t.siting; f.depth = t.depth;
    }
    return f;
}

// -y4m_pixel_format: the C value of a Y4M header, read by the library's own header parser; false: not one of the accepted values
const char* const Y4M_PIXEL_FORMATS = "420jpeg, 420mpeg2, 422, 444, or 420pN, 422pN, 444pN with N in 9, 10, 12, 14, 16";
bool y4m_pixel_format_layout(const std::string& tag, fav_yuv_layout* out)
{
    if (tag.empty() || tag == "420" || tag.find(' ') != std::string::npos) return false;
    const std::string line = "YUV4MPEG2 W2 H2 C" + tag + "\n";
    fav_y4m_stream_header h;
    if (fav_y4m_parse_stream_header_host(line.c_str(), line.size(), &h)) return false;
    *out = h.layout;
    return true;
}

// the C value of a layout, as the header will carry it
std::string y4m_tag_of(const fav_yuv_layout& l)
{
    std::string t = l.chroma == FAV_YUV_444 ? "444" : l.chroma == FAV_YUV_422 ? "422" : l.depth > 8 ? "420" : l.siting == FAV_YUV_SITING_LEFT ? "420mpeg2" : "420jpeg";
    return l.depth > 8 ? t + "p" + std::to_string(l.depth) : t;
}
// -original_colors 1 writes the planes of fav_stream_encode_yuv_colors: 8-bit 4:2:0 / 4:4:4
bool y4m_colors_can_write(const fav_yuv_layout& l) { return l.depth == 8 && l.chroma != FAV_YUV_422; }
std::string y4m_colors_refusal(const fav_yuv_layout& l)
{
    return "-original_colors 1 cannot be combined with the output format " + y4m_tag_of(l) + ": the colour transfer writes 8-bit 4:2:0 / 4:4:4 planes only";
}

struct Counters { std::atomic<long long> png_bytes{0}, cpu_loaders_us{0}, cpu_writers_us{0}, cpu_writer_sync_us{0}; };

// compute queue; upload queue (the next frame's inputs travel while this frame computes); download queue (the 8-bit frame leaves
// while the next frame computes: on the compute queue the 2.8 MB copy held back the next frame's kernels for its whole duration)
// (three queues besides the library's two look-ahead queues: a process gets four hardware queues by default, and the 4-argument
//  mode lost 20 % when a sixth stream made its side queues share one with the compute queue)
struct Queues {
    fav::queue_h compute = favl::queue_create(), upload = favl::queue_create(), download = favl::queue_create();
    void drain() { for (hipStream_t q : {compute.get(), upload.get(), download.get()}) (void)hipStreamSynchronize(q); }
};

// Host pipeline: DEPTH loader threads read + decode frames i+1.. while the GPU works on frame i; decoded
// inputs are copied into pinned staging sets so the H2D copies are true async DMA.
struct Loader {
    static constexpr int DEPTH = 6;
    const Opt& o; const favp::Poll& poll;
    favy::Reader* const y4m; const size_t y4m_bytes;       // -input_y4m: one sequential reader behind the loader threads (else null)
    const int start, end, inc; const bool first_is_single; // the frame range (core:189-191); has frame `start` no prior?
    std::atomic<long long>* const cpu_us;
    size_t pin_px = 0;                       // capacity of a pinned staging set in pixels (0: none yet, loads go to malloc'ed memory)
    double t_wait = 0;
    int next_to_issue, sets_used = 0;
    Pinned pin[DEPTH + 1];
    std::vector<FrameIn> ready = std::vector<FrameIn>(DEPTH + 1);
    std::deque<std::pair<int, std::future<void>>> inflight;      // (slot set, completion of its load)
    // persistent loader threads (a std::thread per frame cost ~0.1 ms of CPU each); no more of them than CPUs to run them on.
    // Declared last: the threads are gone before the staging sets they fill
    Pool pool;

    Loader(const Opt& o_, const favp::Poll& poll_, favy::Reader* y4m_, size_t y4m_bytes_, int start_, int end_, int inc_, bool first_is_single_,
           std::atomic<long long>* cpu_us_, int device)
        : o(o_), poll(poll_), y4m(y4m_), y4m_bytes(y4m_bytes_), start(start_), end(end_), inc(inc_), first_is_single(first_is_single_), cpu_us(cpu_us_),
          next_to_issue(start_), pool(std::min(DEPTH, std::max(2, favl::effective_cpus())), device) {}

    bool idx_ok(int i) const { return inc < 0 ? i >= end : i <= end; }
    FrameIn load(int i, bool first_of_run, const Pinned* pd) { return load_frame_inputs(o, poll, i, first_of_run, pd, pin_px, y4m, y4m_bytes); }
    FrameIn load_pinned(int i, bool first_of_run, int set)
    {
        Pinned& p = pin[set];
        if (pin_px && !p.frame && !p.yuv) {      // first use of this staging set: pinned here, by the loader thread that owns it
            if (y4m) p.yuv = favl::host_alloc<uint8_t>(y4m_bytes); else p.frame = favl::host_alloc<uint8_t>(pin_px * 3);
            if (o.i("estimate_flow") == 0) {                     // (-estimate_flow: frames only)
                p.bw = favl::host_alloc<float>(pin_px * 8);
                if (!o.s("forward_flow_pattern").empty()) p.fw = favl::host_alloc<float>(pin_px * 8); else p.cert = favl::host_alloc<uint8_t>(pin_px);
            }
        }
        return load(i, first_of_run, pin_px ? &p : nullptr);
    }
    void issue()                                                 // keep DEPTH loads in flight
    {
        while ((int)inflight.size() < DEPTH && idx_ok(next_to_issue)) {
            const int i = next_to_issue, set = sets_used % (DEPTH + 1);
            const bool fo = (i == start) && first_is_single;
            auto done_p = std::make_shared<std::promise<void>>();
            inflight.emplace_back(set, done_p->get_future());
            pool.submit([this, i, fo, set, done_p] {
                const double c0 = thread_cpu_seconds();
                ready[set] = load_pinned(i, fo, set);
                *cpu_us += (long long)(1e6 * (thread_cpu_seconds() - c0));
                done_p->set_value();
            });
            next_to_issue += inc; ++sets_used;
        }
    }
    bool pop_next(FrameIn& out)
    {
        if (inflight.empty()) return false;
        const auto tl = std::chrono::steady_clock::now();
        const int set = inflight.front().first;
        inflight.front().second.get(); inflight.pop_front();
        out = ready[set];
        t_wait += std::chrono::duration<double>(std::chrono::steady_clock::now() - tl).count();
        return out.ok;
    }
    void finish() { for (auto& pr : inflight) pr.second.get(); for (auto& r : ready) if (r.index >= 0) r.release(); }
};

// Device input sets: frame i (in use) + up to two frames of look-ahead + one being refilled
struct DevInputs {
    static constexpr int N = 4;
    struct Set { fav::dev_ptr<uint8_t> frame, cert, yuv; fav::dev_ptr<float> bw, fw; fav::event_h up; };
    Set set[N];
    int W = 0, H = 0; size_t yuv_bytes = 0; fav_yuv_layout fmt_in{};        // -input_y4m: a frame's planes and their format
    DevInputs() { for (Set& s : set) s.up = favl::event_create(hipEventDisableTiming | hipEventDisableSystemFence); }
    void alloc(int W_, int H_)
    {
        W = W_; H = H_;
        const size_t n = (size_t)W * H;
        for (Set& s : set) {
            s.frame = favl::dev_alloc<uint8_t>(n * 3); s.cert = favl::dev_alloc<uint8_t>(n); s.bw = favl::dev_alloc<float>(n * 8); s.fw = favl::dev_alloc<float>(n * 8);
            if (yuv_bytes) s.yuv = favl::dev_alloc<uint8_t>(yuv_bytes);
        }
    }
    const Set& before(int k) const { return set[(k + N - 1) % N]; }       // the previous frame in processing order
    // async H2D of one frame's inputs (pinned -> device) on the copy queue; compute != null: everything enqueued on that queue from
    // here on sees them
    void upload(const FrameIn& f, int k, hipStream_t copy, hipStream_t compute)
    {
        const size_t n = (size_t)W * H; const Set& dv = set[k];
        if (f.yuv) {          // -input_y4m: the planes travel, and become the P6 payload on the device, still on the upload queue
            hipMemcpyAsync(dv.yuv.get(), f.yuv, yuv_bytes, hipMemcpyHostToDevice, copy);
            check(fav_yuv_layout_to_rgb8(dv.yuv.get(), W, H, &fmt_in, dv.frame.get(), copy), "fav_yuv_layout_to_rgb8");
        } else hipMemcpyAsync(dv.frame.get(), f.frame, n * 3, hipMemcpyHostToDevice, copy);
        if (f.bw) hipMemcpyAsync(dv.bw.get(), f.bw, n * 8, hipMemcpyHostToDevice, copy);
        if (f.fw) hipMemcpyAsync(dv.fw.get(), f.fw, n * 8, hipMemcpyHostToDevice, copy);
        if (f.cert) hipMemcpyAsync(dv.cert.get(), f.cert, n, hipMemcpyHostToDevice, copy);
        hipEventRecord(dv.up.get(), copy);
        if (compute) hipStreamWaitEvent(compute, dv.up.get(), 0);
    }
};

// -scene_cut: per device input set one host-mapped record that fav_scene_change_rgb8 fills behind the set's upload.  The host
// needs `total` only, which the measure's last kernel stores last: it is set to PENDING (no total exceeds 2^29) when the
// measure is enqueued and polled when the frame's turn comes, a frame later -- like the PNG's size word, without an event.
struct SceneCut {
    static constexpr uint32_t PENDING = 0xFFFFFFFFu;
    struct Close { void operator()(FILE* f) const { fclose(f); } };
    const double T; const bool on;
    fav::host_ptr<fav_scene_change> h; fav::dev_ptr<void> ws;
    std::unique_ptr<FILE, Close> log;
    explicit SceneCut(const Opt& o) : T(o.d("scene_cut")), on(T > 0.0)
    {
        if (o.s("scene_cut_log").empty()) return;
        mkdirs_for(o.s("scene_cut_log"));
        log.reset(fopen(o.s("scene_cut_log").c_str(), "w"));
        if (!log) die("cannot open " + o.s("scene_cut_log"));
    }
    void alloc()
    {
        void* p = nullptr; void* w = nullptr;
        if (hipHostMalloc(&p, DevInputs::N * sizeof(fav_scene_change), hipHostMallocDefault) != hipSuccess ||
            hipMalloc(&w, fav_scene_change_workspace_bytes()) != hipSuccess) die("hipMalloc failed");
        h.reset(static_cast<fav_scene_change*>(p)); ws.reset(w);
    }
    // behind the upload of set k, on its queue: the frame before it in processing order is in the set before it
    void measure(const DevInputs& dev, int k, hipStream_t copy)
    {
        h.get()[k].total = PENDING;
        check(fav_scene_change_rgb8(dev.before(k).frame.get(), dev.set[k].frame.get(), dev.W, dev.H, ws.get(), fav_scene_change_workspace_bytes(),
                                    &h.get()[k], copy), "fav_scene_change_rgb8");
    }
    // is frame i (in set k) a cut?  Its measure was enqueued a frame ago, behind its upload; the first frame has nothing in front of it
    bool decide(int i, int k, bool has_predecessor, const DevInputs& dev, hipStream_t copy)
    {
        uint32_t total = 0; double score = 0.0; bool cut = false;
        if (has_predecessor) {
            volatile uint32_t* tw = &h.get()[k].total;
            for (int spins = 0; *tw == PENDING; ++spins) {
                usleep(50);
                if ((spins & 2047) == 2047) {             // every ~0.1 s: has the GPU faulted? (a query, not a marker)
                    const hipError_t e = hipStreamQuery(copy);
                    if (e != hipSuccess && e != hipErrorNotReady) die("GPU error while measuring a scene change");
                }
            }
            total = *tw;
            score = (double)total / (2.0 * (double)dev.W * (double)dev.H);
            cut = score > T;
        }
        if (log) fprintf(log.get(), "%d %u %.6f %d\n", i, total, score, cut ? 1 : 0);
        return cut;
    }
};

// Where a stylised frame goes.  Frames alternate between two sets of what a sink keeps per frame (k = 0 | 1): frame i + 2 is enqueued
// after the host has seen frame i complete.  Per frame the loop calls, in this order: after_frame (behind the frame's network, with
// the pinned slot the frame will leave through), hand_off (behind the look-ahead and the wait for the frame before), and a frame
// later wait, target and writer_task.
// -original_colors 1: after_frame also gets the device RGB8 frame the network has just consumed, and what it enqueues is the stylised
// frame's luminance on that frame's colours (fav_stream_encode_*_colors, fav_color_transfer_rgb8) instead of the state itself.
struct SinkEnv { const Opt& o; hipStream_t st, st_down; Slots* slots; Counters* cnt; };
class Sink {
public:
    explicit Sink(const SinkEnv& e) : env(e), colors(e.o.i("original_colors") != 0) {}
    virtual ~Sink() = default;
    // QUIET synchronisation: nothing but kernels ever enters the compute queue (DevicePng below says why and how)
    virtual bool quiet() const { return false; }
    virtual size_t setup(fav_stream* fs, int Wo, int Ho) = 0;      // at the known output size; returns the bytes of a pinned slot
    virtual void slot_added(uint8_t*) {}
    virtual uint8_t* frame_out(int) { return nullptr; }            // where the network is to leave the 8-bit frame, if anywhere
    virtual void after_frame(int k, uint8_t* hb, const uint8_t* frame) = 0;
    virtual void hand_off(int k, uint8_t* hb) = 0;
    virtual void wait(int k) = 0;                                  // until frame k is complete where the writer task needs it
    virtual std::string target(int index) = 0;                     // what "Writing output image to" names
    virtual std::function<void()> writer_task(int k, uint8_t* hb, const std::string& path) = 0;
protected:
    std::string png_target(int index) const
    {
        char nm[4096]; snprintf(nm, sizeof nm, "%s-%05d.png", env.o.s("output_prefix").c_str(), index);       // fav.lua:161
        mkdirs_for(nm);
        return nm;
    }
    // events the HOST waits on: blocking (the waiting thread sleeps instead of spinning -- a spinning wait costs one core per waiter,
    // 1.9 ms of CPU per frame for the main thread alone at 530 frames/s) and with the system-scope fence (the host reads what they cover)
    static fav::event_h host_event() { return favl::event_create(hipEventDisableTiming | hipEventBlockingSync); }
    void wait_host_event(hipEvent_t e) const { if (wait_event_sleeping(e) != hipSuccess) die("GPU error while stylising a frame"); }
    // -original_colors into a PNG: no stream format names the matrix, so it is the Y4M header parser's rule for the frame's height
    // (-y4m_matrix overrides)
    int png_colors_matrix() const { return y4m_layout_of(env.o, nullptr, Ho, false).matrix; }
    SinkEnv env; const bool colors; fav_stream* fs = nullptr; int Wo = 0, Ho = 0;
};

// -png_encoder gpu (default): the PNG file's bytes are produced on the device (fav_stream_encode_png: Sub filter + fixed-Huffman /
// run-length deflate per row + Adler-32 / CRC-32 combine), leave as ONE exact-size DMA and the writer thread only write()s them.
// QUIET synchronisation (with the 4-argument look-ahead as well): nothing but kernels ever enters the compute queue.  On this runtime
// a marker behind long-running kernels (hipEventRecord on the compute stream) or a device-side dependency between queues
// (hipStreamWaitEvent, a copy in front of kernels in one stream) is resolved by a runtime thread that SPINS until the marker
// fires -- one core per process, 1.6 ms of CPU per 1.8 ms frame (scripts/runtime_thread_bench.hip, profiles/r03k_runtime_thread.log:
// kernels only 0.03 cores in the background, + one event record per frame 0.70, + a cross-stream dependency 0.74).  So: uploads are
// DMA copies on their own queue and the HOST checks (sleeping poll on that queue's event) that frame i's inputs have arrived before
// it enqueues frame i's kernels -- they were requested a frame earlier; the frame's last kernel writes the PNG size into host-mapped
// memory, which the host polls; the PNG bytes then leave as one DMA on a third queue.  The 4-argument look-ahead (its mask pipeline
// runs a frame ahead on the library's side queues) is started after the host has seen that frame's upload finish and is waited
// for on the host as well (fav_stream_set_host_ordered): no event there either.
// The download queue carries nothing but the files' bytes: they never sit behind the NEXT frame's size word there (that one would wait
// for the next frame's kernels: the writer thread then waited a whole frame for a 0.1 ms DMA).
class DevicePng : public Sink {
public:
    explicit DevicePng(const SinkEnv& e) : Sink(e), overlap(e.o.i("png_overlap") != 0) {}
    bool quiet() const override { return true; }
    size_t setup(fav_stream* fs_, int Wo_, int Ho_) override
    {
        fs = fs_; Wo = Wo_; Ho = Ho_;
        if (Wo > 9000) die("-png_encoder gpu encodes rows of up to 9000 pixels (one image row lives in a CU's LDS); pass -png_encoder host for " + std::to_string(Wo) + "-wide frames");
        cap = fav_png_capacity(Wo, Ho);
        for (auto& d : d_png) d = favl::dev_alloc<uint8_t>(cap);
        h_size = favl::host_alloc<uint32_t>(64);
        return cap;
    }
    // per pinned output slot the event of the exact-size copy into it
    void slot_added(uint8_t* p) override { slot_ev[p] = favl::event_create(hipEventDisableTiming); }
    void after_frame(int k, uint8_t*, const uint8_t* frame) override
    {
        // two frames ago this buffer's bytes left through the download queue: that copy must have finished (it has, long ago)
        if (copy_ev[k] && wait_event_sleeping(copy_ev[k], 50) != hipSuccess) die("GPU error while downloading a frame");
        h_size.get()[k] = 0u;                    // the frame's last kernel overwrites it with the file size (host-mapped)
        // -original_colors 1: one kernel in front of the encoder's, still nothing but kernels on the compute queue; the synchronous
        // encode whatever -png_overlap says (the asynchronous one reads the state on another queue, and has measured no gain)
        if (colors) check(fav_stream_encode_png_colors(fs, frame, png_colors_matrix(), d_png[k].get(), cap, &h_size.get()[k], env.st), "fav_stream_encode_png_colors");
        // -png_overlap 1: on the stream's encoder queue, next to frame i + 1's network -- the host learns of the file
        // through its size word either way
        else if (overlap) check(fav_stream_encode_png_async(fs, d_png[k].get(), cap, &h_size.get()[k], env.st), "fav_stream_encode_png_async");
        else check(fav_stream_encode_png(fs, d_png[k].get(), cap, &h_size.get()[k], env.st), "fav_stream_encode_png");
    }
    void hand_off(int, uint8_t*) override {}     // the bytes leave once their number is known: writer_task
    void wait(int k) override
    {
        // the frame's last kernel (png_finish_kernel) stores the file size into host-mapped memory behind a system-scope fence
        volatile uint32_t* sz = &h_size.get()[k];
        for (int spins = 0; *sz == 0u; ++spins) {
            usleep(100);
            if ((spins & 1023) == 1023) {                 // every ~0.1 s: has the GPU faulted? (a query, not a marker)
                const hipError_t e = hipStreamQuery(env.st);
                if (e != hipSuccess && e != hipErrorNotReady) die("GPU error while stylising a frame");
            }
        }
    }
    std::string target(int index) override { return png_target(index); }
    std::function<void()> writer_task(int k, uint8_t* hb, const std::string& path) override
    {
        // the size word has arrived: ONE DMA of exactly the file's bytes, then the writer thread only write()s
        const uint32_t nbytes = h_size.get()[k];
        if (nbytes < 57 || nbytes > cap) die("fav_stream_encode_png returned an impossible size");
        hipEvent_t cev = slot_ev[hb].get();
        if (hipMemcpyAsync(hb, d_png[k].get(), nbytes, hipMemcpyDeviceToHost, env.st_down) != hipSuccess || hipEventRecord(cev, env.st_down) != hipSuccess) die("D2H of the PNG failed");
        copy_ev[k] = cev;
        env.cnt->png_bytes += nbytes;
        Slots* sl = env.slots; Counters* cnt = env.cnt;
        return [hb, path, nbytes, cev, sl, cnt] {
            const double c0 = thread_cpu_seconds();
            if (wait_event_sleeping(cev, 50) != hipSuccess) { fprintf(stderr, "GPU error while downloading %s\n", path.c_str()); exit(1); }
            cnt->cpu_writer_sync_us += (long long)(1e6 * (thread_cpu_seconds() - c0));
            const int fd = open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0666);
            size_t off = 0;
            while (fd >= 0 && off < nbytes) { const ssize_t n = write(fd, hb + off, nbytes - off); if (n <= 0) break; off += (size_t)n; }
            if (fd < 0 || off != nbytes || close(fd)) { fprintf(stderr, "cannot write %s\n", path.c_str()); exit(1); }
            cnt->cpu_writers_us += (long long)(1e6 * (thread_cpu_seconds() - c0));
            sl->give(hb);
        };
    }
private:
    const bool overlap;
    size_t cap = 0;
    fav::dev_ptr<uint8_t> d_png[2];              // device PNG buffers, alternating
    fav::host_ptr<uint32_t> h_size;              // their sizes, host-mapped
    hipEvent_t copy_ev[2] = {nullptr, nullptr};  // last copy OUT of d_png[k]: the next encode into it waits for this
    std::map<uint8_t*, fav::event_h> slot_ev;
};

// -png_encoder host: the 8-bit frame is downloaded and deflated by zlib on the writer threads (-png_level; ~25 ms per frame and core).
// The frame is complete on the compute queue (ev_out) and leaves on the download queue, which tells the host (ev_done).
class HostPng : public Sink {
public:
    using Sink::Sink;
    size_t setup(fav_stream* fs_, int Wo_, int Ho_) override
    {
        fs = fs_; Wo = Wo_; Ho = Ho_;
        for (auto& d : d_out8) d = favl::dev_alloc<uint8_t>((size_t)Wo * Ho * 3);
        if (colors) d_state = favl::dev_alloc<float>((size_t)Wo * Ho * 12);
        return (size_t)Wo * Ho * 3;
    }
    // -original_colors 1: the network is not asked for its own 8-bit frame; the buffer is filled from the state behind it
    uint8_t* frame_out(int k) override { return colors ? nullptr : d_out8[k].get(); }
    void after_frame(int k, uint8_t*, const uint8_t* frame) override
    {
        if (colors) {         // the operator takes planes the caller owns: a copy of the state (this sink's queue carries copies and events anyway)
            check(fav_stream_get_state(fs, d_state.get(), env.st), "fav_stream_get_state");
            check(fav_color_transfer_rgb8(d_state.get(), frame, Wo, Ho, png_colors_matrix(), d_out8[k].get(), env.st), "fav_color_transfer_rgb8");
        }
        hipEventRecord(ev_out[k].get(), env.st);       // the frame's 8-bit image is complete on the compute queue ...
    }
    void hand_off(int k, uint8_t* hb) override
    {
        hipStreamWaitEvent(env.st_down, ev_out[k].get(), 0);                                       // ... and leaves on the download queue
        hipMemcpyAsync(hb, d_out8[k].get(), (size_t)Wo * Ho * 3, hipMemcpyDeviceToHost, env.st_down);
        hipEventRecord(ev_done[k].get(), env.st_down);
    }
    void wait(int k) override { wait_host_event(ev_done[k].get()); }
    std::string target(int index) override { return png_target(index); }
    std::function<void()> writer_task(int, uint8_t* hb, const std::string& path) override
    {
        const int w = Wo, h = Ho, lvl = env.o.i("png_level");
        Slots* sl = env.slots; Counters* cnt = env.cnt;
        return [hb, path, w, h, lvl, sl, cnt] {
            const double c0 = thread_cpu_seconds();
            if (fav_write_png_rgb8_host(path.c_str(), hb, w, h, lvl)) fprintf(stderr, "%s\n", fav_last_error());
            cnt->cpu_writers_us += (long long)(1e6 * (thread_cpu_seconds() - c0));
            sl->give(hb);                                     // only now may the slot receive another frame
        };
    }
private:
    fav::dev_ptr<uint8_t> d_out8[2];
    fav::dev_ptr<float> d_state;                 // -original_colors 1: the state's planes for fav_color_transfer_rgb8
    fav::event_h ev_out[2] = {favl::event_create(hipEventDisableTiming | hipEventDisableSystemFence), favl::event_create(hipEventDisableTiming | hipEventDisableSystemFence)};
    fav::event_h ev_done[2] = {host_event(), host_event()};
};

// -output_y4m: no PNG at all.  The planes are written by the frame's last kernel straight into a pinned output slot
// (fav_stream_encode_yuv_layout), the host learns of them through an event on the compute queue -- the event-ordered path of
// -png_encoder host, minus its download -- and ONE writer thread write()s the slots in frame order.
class Y4mOut : public Sink {
public:
    // in_header, in_fmt: those of -input_y4m, null without it
    Y4mOut(const SinkEnv& e, const fav_y4m_stream_header* in_header, const fav_yuv_layout* in_fmt) : Sink(e), in_header_(in_header), in_fmt_(in_fmt) {}
    size_t setup(fav_stream* fs_, int Wo_, int Ho_) override
    {
        fs = fs_; Wo = Wo_; Ho = Ho_;
        // the stream's header: the input's (or F25:1 Ip A1:1) with the stylised frames' size and the output's format
        const std::string path = env.o.s("output_y4m");
        fav_y4m_stream_header oh;
        if (in_header_) oh = *in_header_;
        else { memset(&oh, 0, sizeof oh); oh.fps_num = 25; oh.fps_den = 1; oh.interlace = 'p'; oh.aspect_num = oh.aspect_den = 1; }
        fmt_out = y4m_layout_of(env.o, in_fmt_, Ho, true);
        if (colors && !y4m_colors_can_write(fmt_out)) die(y4m_colors_refusal(fmt_out));      // (the input's format: known only now)
        fmt_colors = fav_yuv_format{fmt_out.chroma, fmt_out.siting, fmt_out.matrix, fmt_out.full_range};
        oh.W = Wo; oh.H = Ho; oh.layout = fmt_out;
        bytes = fav_yuv_layout_frame_bytes(Wo, Ho, &fmt_out);
        if (!bytes) die(std::string("-output_y4m: ") + fav_last_error());
        if (path != "-") mkdirs_for(path);
        if (!writer.open(path)) die("Could not open " + path + " for writing");
        if (!writer.header(oh)) die("cannot write the stream header to " + path + ": " + fav_last_error());
        return bytes;
    }
    void after_frame(int, uint8_t* hb, const uint8_t* frame) override      // into the pinned slot
    {
        if (colors) check(fav_stream_encode_yuv_colors(fs, frame, &fmt_colors, hb, bytes, env.st), "fav_stream_encode_yuv_colors");      // the output format's matrix
        else check(fav_stream_encode_yuv_layout(fs, &fmt_out, hb, bytes, env.st), "fav_stream_encode_yuv_layout");
    }
    void hand_off(int k, uint8_t*) override { hipEventRecord(ev_done[k].get(), env.st); }    // nothing to download: the planes are in host memory when this event fires
    void wait(int k) override { wait_host_event(ev_done[k].get()); }
    std::string target(int index) override { return env.o.s("output_y4m") + " (frame " + std::to_string(index) + ")"; }
    std::function<void()> writer_task(int, uint8_t* hb, const std::string& path) override
    {
        // the planes are in the pinned slot (the event covers them): `FRAME` and the payload, behind the frames before it
        favy::Writer* wr = &writer; const size_t nbytes = bytes;
        Slots* sl = env.slots; Counters* cnt = env.cnt;
        return [hb, path, nbytes, wr, sl, cnt] {
            const double c0 = thread_cpu_seconds();
            if (!wr->frame(hb, nbytes)) { fprintf(stderr, "cannot write %s\n", path.c_str()); exit(1); }
            cnt->cpu_writers_us += (long long)(1e6 * (thread_cpu_seconds() - c0));
            sl->give(hb);
        };
    }
private:
    const fav_y4m_stream_header* in_header_; const fav_yuv_layout* in_fmt_;
    favy::Writer writer; fav_yuv_layout fmt_out{}; fav_yuv_format fmt_colors{}; size_t bytes = 0;
    fav::event_h ev_done[2] = {host_event(), host_event()};
};

struct StreamDestroy { void operator()(fav_stream* s) const { fav_stream_destroy(s); } };

// One video: the loop of run_fast_neural_video (core.lua:189-229) with the video CLI's callbacks (fav.lua:93-172).
// `net` / `net_img` live on the current device; `nwriters` PNG threads are the budget.
// The members are destroyed in reverse order of declaration, and that order is meant: the two thread pools (`writers` here, the
// loader's own) go before the pinned memory their tasks touch, the library's stream before the device buffers its side queues read.
// The three queues are declared FIRST and so go last; run() drains them itself once the last frame is written, before anything is freed.
class StreamRun {
public:
    StreamRun(const Opt& o, const fav_flow_opts_ex3& flow_opts, fav_net* net, fav_net* net_img, int nwriters);
    void run(StreamResult* res);
private:
    struct Pending { bool valid = false; int index = 0; bool single = false; uint8_t* hb = nullptr; int k = 0; std::chrono::steady_clock::time_point t0; };
    static int current_device() { int d = 0; (void)hipGetDevice(&d); return d; }
    static favp::Poll poll_of(const Opt& o) { favp::Poll p; p.timeout_s = o.d("poll_timeout"); p.settle_s = std::max(0.0, o.d("poll_settle")); p.out = favl::msg(); return p; }
    bool load_resume_state();
    void setup(const FrameIn& cur, int i);
    void top_up(int i);
    void enqueue_network(FrameIn& cur, int i, uint8_t* d_out8);
    void finish(Pending& pd);
    uint8_t* new_slot();
    void write_temporal_eval() const;

    const Opt& o; const fav_flow_opts_ex3& flow_opts; fav_net* const net; fav_net* const net_img;
    const bool estimate;                     // the flows come from the frames (and go through the fused check)
    const bool fused_check, teval, backward;
    const int border, structure;
    const int start, end, inc;               // core:189-191
    const favp::Poll poll;
    const int device = current_device();
    const double cpu0 = process_cpu_seconds(), cpu_main0 = thread_cpu_seconds();
    Counters cnt;
    Queues q;
    hipStream_t const st = q.compute.get(), st_copy = q.upload.get(), st_down = q.download.get();
    favy::Reader y4m_reader;                 // -input_y4m: one sequential reader behind the loader threads
    int W = 0, H = 0;                        // frame size
    int Wo = 0, Ho = 0;                      // size of the stylised frames: the network's output (H x W when both are multiples of 4)
    DevInputs dev;
    fav::dev_ptr<void> d_flow_ws; size_t flow_ws_bytes = 0;
    std::vector<int> long_term; bool lt_frame_seen = false;      // -long_term: {1, d...} (empty: off) | the library's history holds the previous FRAME
    fav::dev_ptr<float> d_prev, d_cur; std::vector<double> temporal;      // -temporal_eval_file
    SceneCut scene;
    // continue_with > 1: the previous stylised PNG as the recurrent state, rW x rH
    std::vector<float> resume_state; int rW = 0, rH = 0;
    const bool have_resume = load_resume_state();
    // pinned output slots in flight to the PNG pool (deflate ~55 ms/frame/thread), allocated on demand, at most nslots
    Slots slots; std::vector<fav::host_ptr<uint8_t>> h_out; size_t slot_bytes = 0; int nslots = 0;
    std::unique_ptr<Sink> sink;
    bool quiet = false;
    std::unique_ptr<fav_stream, StreamDestroy> fs;
    std::unique_ptr<Loader> loader;
    std::unique_ptr<Pool> writers;
    // Look-ahead: frames i+1 .. i+LA are uploaded (device set of ahead[k] = dset + 1 + k) and, with the checker's 4-argument mode, their
    // masks are under way on the side queues while frame i is enqueued.  That mode needs TWO frames: a mask takes 1.5 ms behind a
    // 0.45 ms upload, a frame 1.9 ms -- one frame ahead, every frame waited 0.1 ms for its mask (period 2.05 ms: 460 frames/s;
    // profiles/r03z_cli_4arg_trace.txt)
    const int LA;
    std::deque<FrameIn> ahead; bool drained = false;
    int done = 0, dset = 0;
    double t_wait_writer = 0;
    std::chrono::steady_clock::time_point t_begin;
    double setup_s = 0;
};

// -long_term: the list of distances beyond 1 -> {1, d...}; false: malformed (not ascending integers in 2..16, more than three, empty items)
static bool parse_long_term(const std::string& v, std::vector<int>& out)
{
    out.assign(1, 1);
    if (v.empty()) { out.clear(); return true; }
    for (size_t a = 0; a <= v.size();) {
        const size_t b = std::min(v.find(',', a), v.size());
        const std::string item = v.substr(a, b - a);
        if (item.empty() || item.size() > 2 || item.find_first_not_of("0123456789") != std::string::npos) return false;
        const int d = atoi(item.c_str());
        if (d <= out.back() || d > FAV_LONG_TERM_MAX_DISTANCE || (int)out.size() >= FAV_LONG_TERM_MAX) return false;
        out.push_back(d);
        a = b + 1;
    }
    return true;
}

StreamRun::StreamRun(const Opt& o_, const fav_flow_opts_ex3& fo, fav_net* net_, fav_net* net_img_, int nwriters)
    : o(o_), flow_opts(fo), net(net_), net_img(net_img_), estimate(o.i("estimate_flow") != 0), fused_check(estimate || !o.s("forward_flow_pattern").empty()),
      teval(!o.s("temporal_eval_file").empty()), backward(o.f("backward")), border(o.s("warp_border") == "cpu" ? FAV_BORDER_CPU : FAV_BORDER_STN),
      structure(o.i("structure")), start(backward ? o.i("num_frames") - 1 : o.i("continue_with")), end(backward ? 1 : o.i("num_frames")), inc(backward ? -1 : 1),
      poll(poll_of(o)), scene(o), LA((fused_check && !estimate && structure != 0) ? 2 : 1)
{
    const bool y4m_in = !o.s("input_y4m").empty();
    if (y4m_in) {
        const std::string err = y4m_reader.open(o.s("input_y4m"));
        if (!err.empty()) die(err);
        const fav_y4m_stream_header& h = y4m_reader.header();
        dev.fmt_in = y4m_layout_of(o, &h.layout, h.H, false);
        dev.yuv_bytes = fav_yuv_layout_frame_bytes(h.W, h.H, &dev.fmt_in);
        if (!dev.yuv_bytes) die(std::string("-input_y4m: ") + fav_last_error());
        y4m_reader.set_frame_bytes(dev.yuv_bytes);
    }
    // the output mode is chosen here, once: a sink each (above), and the writer threads it can use
    const SinkEnv env{o, st, st_down, &slots, &cnt};
    if (!o.s("output_y4m").empty()) {
        sink.reset(new Y4mOut(env, y4m_in ? &y4m_reader.header() : nullptr, y4m_in ? &dev.fmt_in : nullptr));
        nwriters = 1;                        // a stream's frames leave in order: the pool's queue is first in, first out
    } else if (o.s("png_encoder") == "gpu") {
        sink.reset(new DevicePng(env));
        if (o.i("writers") <= 0) nwriters = std::min(nwriters, 4);      // they only write() finished files: 0.5 ms per frame
    } else sink.reset(new HostPng(env));
    quiet = sink->quiet();
    writers.reset(new Pool(nwriters, device));
    nslots = nwriters + 2;
    loader.reset(new Loader(o, poll, y4m_in ? &y4m_reader : nullptr, dev.yuv_bytes, start, end, inc, !have_resume && start != 1, &cnt.cpu_loaders_us, device));
}

// continue_with > 1: reload the previous stylised PNG as the recurrent state (8-bit; the reference's
// video CLI does not reload anything and fails, fast_artistic_video.lua:89,153-156); its size is validated against the first frame's
bool StreamRun::load_resume_state()
{
    if (backward || start <= 1 || o.f("create_inconsistent")) return false;
    std::vector<uint8_t> prev;
    char nm[4096]; snprintf(nm, sizeof nm, "%s-%05d.png", o.s("output_prefix").c_str(), start - 1);
    if (!read_png_rgb8(nm, prev, rW, rH)) {
        fprintf(stderr, "warning: %s not found; frame %d is stylised without a prior\n", nm, start);
        return false;
    }
    const size_t n = (size_t)rW * rH;
    resume_state.resize(n * 3);
    for (size_t i = 0; i < n; ++i)
        for (int c = 0; c < 3; ++c) resume_state[(size_t)c * n + i] = prev[i * 3 + c] / 255.0f;
    return true;
}

uint8_t* StreamRun::new_slot()
{
    h_out.push_back(favl::host_alloc<uint8_t>(slot_bytes));
    sink->slot_added(h_out.back().get());
    return h_out.back().get();
}

// the one-time set-up: the first frame (loaded synchronously) sizes every buffer
void StreamRun::setup(const FrameIn& cur, int i)
{
    W = cur.W; H = cur.H;
    fav_stream_opts so{border, o.i("occlusions_min_filter"), o.f("invert_occlusion") ? 1 : 0, o.f("fix_occlusions") ? 1 : 0,
                       o.s("fill_occlusions") == "uniform-random" ? 1 : 0, (unsigned)o.i("seed")};
    fav_stream* s = nullptr;
    check(fav_stream_create(net, H, W, &so, &s), "fav_stream_create");
    fs.reset(s);
    check(fav_stream_output_size(s, &Ho, &Wo), "fav_stream_output_size");
    if (quiet) check(fav_stream_set_host_ordered(s, 1), "fav_stream_set_host_ordered");
    if (have_resume && (rW != Wo || rH != Ho)) die("-continue_with: the previous PNG's size differs from the stylised frames' (" + std::to_string(Wo) + "x" + std::to_string(Ho) + ")");
    if (teval && (Wo != W || Ho != H))
        die("-temporal_eval_file: the stylised frames (" + std::to_string(Wo) + "x" + std::to_string(Ho) + ") are larger than the flow; the reference's func_eval fails on such sizes as well (fav.lua:128-151)");
    if (o.i("original_colors") != 0 && (Wo != W || Ho != H))
        die("-original_colors 1: the stylised frames (" + std::to_string(Wo) + "x" + std::to_string(Ho) + ") are larger than the input frames (" + std::to_string(W) + "x" +
            std::to_string(H) + "): there are no original colours for the added pixels; use a size whose sides are multiples of 4");
    if (net_img) check(fav_stream_set_image_net(s, net_img), "fav_stream_set_image_net");
    parse_long_term(o.s("long_term"), long_term);      // (validated in main)
    if (!long_term.empty()) check(fav_stream_set_long_term(s, long_term.data(), (int)long_term.size()), "-long_term");
    if (o.d("scale_factor") != 1.0) {          // img:view(1, 3, H * f, W * f) (core.lua:130) needs whole numbers
        const double f = o.d("scale_factor"), hs = H * f, ws = W * f;
        if (std::fabs(hs - std::round(hs)) > 1e-9 * hs || std::fabs(ws - std::round(ws)) > 1e-9 * ws || hs < 0.5 || ws < 0.5 || hs > 1e6 || ws > 1e6) {
            char msg[256];
            snprintf(msg, sizeof msg, "-scale_factor %s: %dx%d frames would be stylised at %gx%g; both sides must be whole numbers", o.s("scale_factor").c_str(), W, H, ws, hs);
            die(msg);
        }
        check(fav_stream_set_single_image_size(s, (int)std::round(hs), (int)std::round(ws)), "-scale_factor");
    }
    const size_t n = (size_t)W * H, no = (size_t)Wo * Ho;
    slot_bytes = sink->setup(s, Wo, Ho);
    dev.alloc(W, H);
    // pinned memory is paid for by the page (~0.2 ms per MB): two output slots now, the others when the pool first falls behind;
    // every loader thread pins its own staging set on first use, in parallel with this thread's set-up
    for (int k = 0; k < std::min(2, nslots); ++k) slots.add(new_slot());
    loader->pin_px = n;
    if (have_resume) {
        const auto d_state = favl::dev_alloc<float>(no * 12);
        hipMemcpy(d_state.get(), resume_state.data(), no * 12, hipMemcpyHostToDevice);
        check(fav_stream_set_state(s, d_state.get(), st), "fav_stream_set_state");
        hipStreamSynchronize(st);
    }
    if (scene.on) scene.alloc();
    if (estimate) {
        flow_ws_bytes = fav_flow_pairs_workspace_bytes_ex3(W, H, 1, &flow_opts);      // room for both flows at once: the batch of one
        // -long_term: the flows of every distance and the batch of as many pairs; it also serves the batch of one after -continue_with
        if (flow_ws_bytes && !long_term.empty()) flow_ws_bytes = std::max(flow_ws_bytes, fav_stream_long_term_workspace_bytes(s, &flow_opts));
        if (!flow_ws_bytes) die(std::string("-estimate_flow: ") + fav_last_error());
        d_flow_ws = favl::dev_alloc<void>(flow_ws_bytes);
        if (!cur.single) {                       // -continue_with: the frame before the first one is read as well, into the set "before" dset
            const std::string pp = fmt_int(o.s("input_pattern"), i - inc);
            uint8_t* pf = nullptr; int pw, ph, pch;
            check(fav_read_pnm_host(pp.c_str(), &pf, &pw, &ph, &pch), pp.c_str());
            if (pch != 3 || pw != W || ph != H) die(pp + ": expected a colour (P6) frame of the sequence's size");
            if (hipMemcpy(dev.before(dset).frame.get(), pf, n * 3, hipMemcpyHostToDevice) != hipSuccess) die("upload failed");
            fav_free_host(pf);
        }
    }
    dev.upload(cur, dset, st_copy, quiet ? nullptr : st);
    hipStreamSynchronize(st_copy);               // the first frame's host buffers are malloc'ed: release them now
    setup_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count();     // first frame read + every allocation
}

// frames i+1 (i+2): wait for the loader, upload, and start the consistency mask on the side queues so the (sequential, 1.5 ms)
// 4-argument structure pass overlaps the network of the frames before it
void StreamRun::top_up(int i)
{
    while ((int)ahead.size() < LA && !drained) {
        FrameIn nxt;
        if (!loader->idx_ok(i + inc * ((int)ahead.size() + 1)) || !loader->pop_next(nxt)) { drained = true; break; }
        if (nxt.W != W || nxt.H != H) die("frame size changed inside the sequence");
        const int nset = (dset + 1 + (int)ahead.size()) % DevInputs::N;
        const DevInputs::Set& dn = dev.set[nset];
        dev.upload(nxt, nset, st_copy, quiet ? nullptr : st);
        if (scene.on) scene.measure(dev, nset, st_copy);
        if (fused_check && !estimate && !nxt.single && (!quiet || structure != 0)) {
            // quiet: the look-ahead may only start on inputs the host has seen arrive (0.35 ms of DMA; the GPU is busy with frame i-1)
            if (quiet && wait_event_sleeping(dn.up.get(), 50) != hipSuccess) die("GPU error while uploading a frame");
            check(fav_stream_prefetch_mask(fs.get(), dn.frame.get(), dn.bw.get(), dn.fw.get(), structure, st), "fav_stream_prefetch_mask");
        }
        ahead.push_back(nxt);
    }
}

// frame i's network, in device set dset, behind its inputs
void StreamRun::enqueue_network(FrameIn& cur, int i, uint8_t* d_out8)
{
    const DevInputs::Set& dc = dev.set[dset];
    if (quiet && wait_event_sleeping(dc.up.get(), 50) != hipSuccess) die("GPU error while uploading a frame");      // requested a frame ago: already there
    // a cut takes the path of a frame without a prior: image model, no flow, the recurrence starts afresh
    if (scene.on && scene.decide(i, dset, done > 0, dev, st_copy)) cur.single = true;
    if (teval && !d_prev) { d_prev = favl::dev_alloc<float>((size_t)W * H * 12); d_cur = favl::dev_alloc<float>((size_t)W * H * 12); }
    if (teval && !cur.single) check(fav_stream_get_state(fs.get(), d_prev.get(), st), "fav_stream_get_state");
    if (cur.single) {
        check(fav_stream_first_frame(fs.get(), dc.frame.get(), nullptr, d_out8, st), "fav_stream_first_frame");       // core:203-204
    } else if (estimate && lt_frame_seen) {
        // -long_term: the previous frames are in the library's history; the flows of every distance land at the head of the workspace
        check(fav_stream_next_frame_estimate_lt(fs.get(), dc.frame.get(), &flow_opts, structure, d_flow_ws.get(), flow_ws_bytes, nullptr, d_out8, st),
              "fav_stream_next_frame_estimate_lt");
    } else if (estimate) {
        // the previous frame in processing order is still in the device set before this one: with one frame of look-ahead the
        // uploads only ever touch the set after it
        check(fav_stream_next_frame_estimate_ex3(fs.get(), dc.frame.get(), dev.before(dset).frame.get(), &flow_opts, structure, dc.bw.get(), dc.fw.get(),
                                             d_flow_ws.get(), flow_ws_bytes, nullptr, d_out8, st), "fav_stream_next_frame_estimate");
    } else if (fused_check) {
        check(fav_stream_next_frame_flow(fs.get(), dc.frame.get(), dc.bw.get(), dc.fw.get(), structure, nullptr, d_out8, st), "fav_stream_next_frame_flow");
    } else {
        check(fav_stream_next_frame_cert(fs.get(), dc.frame.get(), dc.bw.get(), dc.cert.get(), nullptr, d_out8, st), "fav_stream_next_frame_cert");   // core:206-208
    }
    const bool lt_ran = estimate && lt_frame_seen && !cur.single;      // (distance 1's backward flow is then the workspace's first field)
    lt_frame_seen = !long_term.empty();
    if (teval) {                                     // fav.lua:128-151 (third number)
        double tl = 0.0;
        if (!cur.single) {
            check(fav_stream_get_state(fs.get(), d_cur.get(), st), "fav_stream_get_state");
            check(fav_temporal_loss_host(d_prev.get(), d_cur.get(), lt_ran ? static_cast<const float*>(d_flow_ws.get()) : dc.bw.get(), fused_check ? fav_stream_last_mask(fs.get()) : dc.cert.get(), H, W, border, &tl, st), "fav_temporal_loss_host");
        }
        temporal.push_back(tl);
    }
}

// the frame before: wait, report, hand to the writer pool
void StreamRun::finish(Pending& pd)
{
    if (!pd.valid) return;
    sink->wait(pd.k);
    check(fav_net_check(net), "stylising a frame");      // a stream-K hand-off that timed out: fail at THIS frame, before its PNG exists
    if (net_img) check(fav_net_check(net_img), "stylising a frame");
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - pd.t0).count();
    if (pd.single) fprintf(favl::msg(), "Elapsed time for stylizing frame independently:%g\n", ms / 1000.0);           // core:155
    else fprintf(favl::msg(), "Elapsed time for stylizing frame:%g\n", ms / 1000.0);                                   // core:177
    const std::string path = sink->target(pd.index);
    fprintf(favl::msg(), "Writing output image to %s\n", path.c_str());
    writers->submit(sink->writer_task(pd.k, pd.hb, path));
    pd.valid = false;
}

void StreamRun::write_temporal_eval() const             // core.lua:231-238 layout: values joined by ';', then the mean
{
    FILE* f = fopen(o.s("temporal_eval_file").c_str(), "a");
    if (!f) die("cannot open " + o.s("temporal_eval_file"));
    double sum = 0.0;
    for (size_t k = 0; k < temporal.size(); ++k) { fprintf(f, "%s%.9g", k ? ";" : "", temporal[k]); sum += temporal[k]; }
    fprintf(f, "\n%.9g\n", sum / (double)temporal.size());
    fclose(f);
}

void StreamRun::run(StreamResult* res)
{
    t_begin = std::chrono::steady_clock::now();
    double t_gpu = 0;
    Pending pend;                                // the host runs one frame ahead of the GPU: frame i is enqueued before frame i-1's completion is awaited
    FrameIn cur = loader->load(start, !have_resume && start != 1, nullptr);      // the first frame is loaded synchronously (its size sizes every buffer)
    loader->next_to_issue = start + inc;
    for (int i = start; loader->idx_ok(i) && cur.ok; i += inc) {                                              // core:196-197
        if (!fs) setup(cur, i);
        else if (cur.W != W || cur.H != H) die("frame size changed inside the sequence");
        loader->issue();
        const auto t0 = std::chrono::steady_clock::now();
        static const bool loop_trace = diag_env("FAV_LOOP_TRACE") != nullptr;      // where a loop iteration's host time goes (frames 100-111)
        double tr_ms[6] = {0, 0, 0, 0, 0, 0};
        auto tr_mark = [&](int k) { if (loop_trace) tr_ms[k] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); };
        tr_mark(0);      // (the look-ahead is topped up BEHIND the frame's enqueue, also for the first frame: its enqueue is 15 ms of one-time
                         //  work -- activation arena, code objects -- that now runs while the loaders read and pin frames 2, 3, ...)
        Pending now; now.valid = true; now.index = i; now.k = done & 1; now.t0 = t0;
        enqueue_network(cur, i, sink->frame_out(now.k));
        now.single = cur.single;
        tr_mark(1);                                      // frame i enqueued
        const auto tw = std::chrono::steady_clock::now();
        now.hb = slots.try_take();                       // a pinned output slot nobody is reading ...
        if (!now.hb) now.hb = (int)h_out.size() < nslots ? new_slot() : slots.take();      // ... a new one while allowed, else wait for the PNG pool
        t_wait_writer += std::chrono::duration<double>(std::chrono::steady_clock::now() - tw).count();
        // -original_colors 1 reads the frame the network has just consumed, dev.set[dset].frame (with -input_y4m: what fav_yuv_to_rgb8
        // left there).  It still holds frame i when the sink's kernels run: they are enqueued here, on the compute queue, behind frame
        // i's network, whose inputs the queue (or, quiet, the host) has seen arrive; and the set is refilled by top_up of the iteration
        // of frame i + N - LA >= i + 2 at the earliest, after finish() in the iteration of frame i + 1 has SEEN frame i complete where
        // the writer needs it -- the size word, the download or the planes, all behind the sink's kernels.
        sink->after_frame(now.k, now.hb, dev.set[dset].frame.get());
        tr_mark(2);                                      // PNG encode enqueued
        top_up(i);                                       // behind frame i's kernels: the 0.45 ms this waits for the upload are not in front of them
        const auto tg = std::chrono::steady_clock::now();
        finish(pend);                                    // frame i-1: wait, report, hand to the PNG pool -- frame i's kernels are already queued
        t_gpu += std::chrono::duration<double>(std::chrono::steady_clock::now() - tg).count();
        tr_mark(3);
        static const bool loop_trace_start = loop_trace && atoi(diag_env("FAV_LOOP_TRACE")) == 2;       // 2: the first 48 frames instead (start-up)
        if (loop_trace_start && done < 48)
            fprintf(stderr, "loop trace frame %d: at %.3f ms since start: look-ahead %.3f  frame enqueued %.3f  encode enqueued %.3f  previous frame finished %.3f ms\n", i,
                    std::chrono::duration<double, std::milli>(t0 - t_begin).count(), tr_ms[0], tr_ms[1], tr_ms[2], tr_ms[3]);
        if (loop_trace && !loop_trace_start && done >= 100 && done < 112)
            fprintf(stderr, "loop trace frame %d: look-ahead %.3f  frame enqueued %.3f  encode enqueued %.3f  previous frame finished %.3f ms\n", i, tr_ms[0], tr_ms[1], tr_ms[2], tr_ms[3]);
        sink->hand_off(now.k, now.hb);
        pend = now;
        if (cur.index >= 0) cur.release();               // malloc'ed (first frame); pinned sets are reused
        ++done;
        if (ahead.empty()) break;
        cur = ahead.front(); ahead.pop_front(); dset = (dset + 1) % DevInputs::N;
    }
    finish(pend);
    const auto t_tail = std::chrono::steady_clock::now();       // the GPU is done: what follows is the PNG pool draining
    loader->finish();
    fflush(favl::msg());
    writers->wait_below(0);
    if (y4m_reader.failed_at()) {                        // -input_y4m; the complete frames before it are written: now it is an error
        fflush(favl::msg());
        die(o.s("input_y4m") + (y4m_reader.failure() == favy::Reader::TRUNCATED ? ": the stream ends inside frame " : ": no FRAME marker (or a read error) at frame ") +
            std::to_string(y4m_reader.failed_at()));
    }
    if (!temporal.empty()) write_temporal_eval();
    res->frames = done; res->setup = setup_s;
    res->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count();
    res->tail = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_tail).count();
    res->wait_loader = loader->t_wait; res->wait_gpu = t_gpu; res->wait_png = t_wait_writer;
    res->cpu_s = process_cpu_seconds() - cpu0; res->png_bytes = cnt.png_bytes.load();
    res->cpu_loaders = 1e-6 * cnt.cpu_loaders_us.load(); res->cpu_writers = 1e-6 * cnt.cpu_writers_us.load(); res->cpu_main = thread_cpu_seconds() - cpu_main0;
    res->cpu_writer_sync = 1e-6 * cnt.cpu_writer_sync_us.load();
    q.drain();           // every frame has been waited for; nothing may still be queued when the members below `q` free what the queues used
}

}  // namespace

int main(int argc, char** argv)
{
    Opt o;
    // fast_artistic_video.lua:21-67 (defaults as there, except -gpu: the reference defaults to the CPU, which this build does not have)
    o.v = {{"model_img", "models/checkpoint-candy-image.t7"}, {"model_vid", "models/checkpoint-candy-video.t7"}, {"num_frames", "9999"}, {"continue_with", "1"},
           {"input_pattern", ""}, {"output_prefix", "out"}, {"flow_pattern", ""}, {"occlusions_pattern", ""},
           {"occlusions_min_filter", "7"}, {"fill_occlusions", "vgg-mean"}, {"median_filter", "3"}, {"scale_factor", "1"},
           {"gpu", "0"}, {"backend", "cuda"}, {"use_cudnn", "1"}, {"cudnn_benchmark", "0"},
           {"flow_pattern_eval", ""}, {"occlusions_pattern_eval", ""}, {"evaluation_file", "evaluation.txt"},
           {"content_weights", "1.0"}, {"content_layers", "16"}, {"loss_network", "models/vgg16.t7"},
           {"style_image", "images/styles/candy.jpg"}, {"style_image_size", "256"}, {"style_weights", "1.0"},
           {"style_layers", "4,9,16,23"}, {"style_target_type", "gram"},
           // additive
           {"forward_flow_pattern", ""}, {"structure", "1"}, {"warp_border", "stn"}, {"poll_timeout", "3600"}, {"poll_settle", "1.0"},
           {"png_level", "1"}, {"png_encoder", "gpu"}, {"png_overlap", "0"}, {"writers", "0"}, {"timing", "0"}, {"temporal_eval_file", ""}, {"seed", "1"}, {"precision", "fp32"},
           {"input_y4m", ""}, {"output_y4m", ""}, {"y4m_matrix", "auto"}, {"y4m_range", "auto"}, {"y4m_format", ""}, {"y4m_pixel_format", ""},
           {"scene_cut", "0"}, {"scene_cut_log", ""}, {"original_colors", "0"}, {"long_term", ""},
           {"estimate_flow", "0"}, {"flow_levels", "0"},      // (the other -flow_* flags: favl::add_flow_flags below)
           {"streams", ""}, {"gpus", "1"}, {"force_dist", "0"}, {"dry_run", "0"}, {"shared_gpu", "0"}, {"pin_workers", "1"},
           // internal (set by the launcher for its workers)
           {"worker_rank", "-1"}, {"worker_world", "0"}, {"rccl_id_file", ""},
           // test hook: -load_probe <i> loads frame i's inputs exactly as the frame loop's loader threads do (polling included), prints one
           // JSON line with a hash of each and exits -- no device is touched (tests/test_cpu_poll.py)
           {"load_probe", "0"}};
    o.b = {{"invert_occlusion", false}, {"fix_occlusions", false}, {"backward", false}, {"create_inconsistent", false},
           {"evaluate", false}, {"invert_occlusion_eval", false}, {"fix_occlusions_eval", false}, {"backward_eval", false}};
    favl::add_flow_flags(o.v);
    for (int a = 1; a < argc; ++a) {
        if (argv[a][0] != '-') die(std::string("invalid argument: ") + argv[a]);
        const std::string k = argv[a] + 1;
        if (o.b.count(k)) { o.b[k] = true; continue; }
        if (!o.v.count(k)) die("unknown option -" + k);
        if (a + 1 >= argc) die("missing value for -" + k);
        o.v[k] = argv[++a];
    }
    // YUV4MPEG2 streams in and / or out: everything that cannot work is refused here, before any device is opened
    const bool y4m_in = !o.s("input_y4m").empty(), y4m_out = !o.s("output_y4m").empty();
    if (o.s("output_y4m") == "-") favl::msg() = stderr;                                                     // stdout carries the stream and nothing else
    if (y4m_in && !o.s("input_pattern").empty()) die("-input_y4m is given INSTEAD of -input_pattern: the frames come from one or the other, not both");
    if (y4m_in && o.f("backward")) die("-backward cannot be combined with -input_y4m: a stream is read from its first frame to its last");
    if ((y4m_in || y4m_out) && o.s("continue_with") != "1")
        die("-continue_with " + o.s("continue_with") + " cannot be combined with -input_y4m / -output_y4m: a stream starts at its first frame");
    if ((o.s("input_y4m") == "-" || o.s("output_y4m") == "-") && favl::split_list(o.s("streams")).size() > 1)
        die("-input_y4m - / -output_y4m - is ONE stream (stdin / stdout): it cannot be combined with more than one -streams entry");
    if (o.s("y4m_matrix") != "auto" && o.s("y4m_matrix") != "bt601" && o.s("y4m_matrix") != "bt709") die("-y4m_matrix must be auto, bt601 or bt709, not '" + o.s("y4m_matrix") + "'");
    if (o.s("y4m_range") != "auto" && o.s("y4m_range") != "limited" && o.s("y4m_range") != "full") die("-y4m_range must be auto, limited or full, not '" + o.s("y4m_range") + "'");
    if (!o.s("y4m_format").empty() && o.s("y4m_format") != "420jpeg" && o.s("y4m_format") != "420mpeg2" && o.s("y4m_format") != "444")
        die("-y4m_format must be 420jpeg, 420mpeg2 or 444, not '" + o.s("y4m_format") + "'");
    fav_yuv_layout asked{};                                                                                  // -y4m_pixel_format: what it names
    if (!o.s("y4m_pixel_format").empty()) {
        if (!o.s("y4m_format").empty()) die("-y4m_format and -y4m_pixel_format both set the output's format: give one of them");
        if (!y4m_pixel_format_layout(o.s("y4m_pixel_format"), &asked))
            die(std::string("-y4m_pixel_format must be ") + Y4M_PIXEL_FORMATS + ", not '" + o.s("y4m_pixel_format") + "'");
    }
    // -original_colors: refused here, before any device is opened
    if (o.s("original_colors") != "0" && o.s("original_colors") != "1") die("-original_colors must be 0 or 1, not '" + o.s("original_colors") + "'");
    if (o.s("original_colors") == "1" && y4m_out && !o.s("y4m_pixel_format").empty() && !y4m_colors_can_write(asked)) die(y4m_colors_refusal(asked));
    if (o.s("original_colors") == "1" && o.i("continue_with") > 1)
        die("-original_colors 1 cannot be combined with -continue_with " + o.s("continue_with") +
            ": -continue_with reloads the previous PNG as the recurrent state, and with -original_colors 1 the PNG is not the state");
    if (!y4m_in && o.s("input_pattern").empty()) die("Must give -input_pattern");                         // fav.lua:177-179
    if (o.s("estimate_flow") != "0" && o.s("estimate_flow") != "1") die("-estimate_flow must be 0 or 1, not '" + o.s("estimate_flow") + "'");
    const bool estimate = o.i("estimate_flow") != 0;
    {   // -scene_cut: the recurrence restarts where the picture changes by more than T (0: off)
        const std::string sc = o.s("scene_cut");
        char* end = nullptr;
        const double T = strtod(sc.c_str(), &end);
        if (sc.empty() || end == sc.c_str() || *end != '\0' || !std::isfinite(T) || T < 0.0 || T > 1.0) die("-scene_cut must be a number in [0, 1] (0: off), not '" + sc + "'");
        if (T > 0.0 && !estimate)
            die("-scene_cut " + sc + " needs -estimate_flow 1: with flows from files the look-ahead has already started a frame's mask when the cut is known");
        if (T > 0.0 && o.f("create_inconsistent")) die("-scene_cut " + sc + " cannot be combined with -create_inconsistent: no frame has a prior there");
        if (!o.s("scene_cut_log").empty() && T == 0.0) die("-scene_cut_log needs -scene_cut: without it no frame is measured");
    }
    if (!o.s("long_term").empty()) {      // -long_term: priors from frames further back than the last
        const std::string lt = o.s("long_term");
        std::vector<int> d;
        if (!parse_long_term(lt, d))
            die("-long_term must list the distances beyond 1: ascending whole numbers in 2.." + std::to_string(FAV_LONG_TERM_MAX_DISTANCE) + ", at most " +
                std::to_string(FAV_LONG_TERM_MAX - 1) + ", separated by commas (e.g. 2,4), not '" + lt + "'");
        if (!estimate) die("-long_term " + lt + " needs -estimate_flow 1: flows from files exist for distance 1 only");
        if (o.f("create_inconsistent")) die("-long_term " + lt + " cannot be combined with -create_inconsistent: no frame has a prior there");
    }
    favl::validate_flow_flags(o.v, estimate, "-estimate_flow 1");
    const fav_flow_opts_ex3 flow_opts = favl::flow_opts_of(o.v);
    if (estimate) {
        for (const char* k : {"flow_pattern", "forward_flow_pattern", "occlusions_pattern"})
            if (!o.s(k).empty()) die(std::string("-estimate_flow 1 computes both flows and the certainty from the frames: it cannot be combined with -") + k);
        if (atof(o.s("scale_factor").c_str()) != 1.0) die("-estimate_flow 1 cannot be combined with a -scale_factor other than 1");
        if (fav_flow_workspace_bytes_ex3(64, 64, &flow_opts) == 0) die(std::string("-flow_alpha / -flow_eps / -flow_iters / -flow_warps / -flow_levels: ") + fav_last_error());
    }
    const bool fused_check = !o.s("forward_flow_pattern").empty();
    if (!estimate && !o.f("create_inconsistent") && (o.s("flow_pattern").empty() || (o.s("occlusions_pattern").empty() && !fused_check)))
        die("Must give -flow_pattern and -occlusions_pattern");                                              // fav.lua:180-182
    if (o.i("gpu") < 0) die("-gpu -1: this build has no CPU backend (the CPU restatement lives in oracle/ and is test infrastructure only)");
    if (o.f("evaluate")) die("-evaluate needs the VGG-16 perceptual-loss network: outside the hot-path scope (DESIGN.md)");
    {   // core.lua:127-130,150-152: frames without a prior are stylised at H*f x W*f and scaled back
        const std::string sf = o.s("scale_factor");
        char* end = nullptr;
        const double f = strtod(sf.c_str(), &end);
        if (sf.empty() || end == sf.c_str() || *end != '\0' || !std::isfinite(f) || f <= 0.0) die("-scale_factor must be a number above 0, not '" + sf + "'");
    }
    if (o.s("fill_occlusions") != "vgg-mean" && o.s("fill_occlusions") != "uniform-random") die("-fill_occlusions must be vgg-mean or uniform-random");
    if (o.s("png_encoder") != "gpu" && o.s("png_encoder") != "host") die("-png_encoder must be gpu (the file's bytes are produced on the device) or host (zlib, -png_level)");
    if (o.s("precision") != "fp32" && o.s("precision") != "bf16") die("-precision must be fp32 (parity mode) or bf16 (bf16 operands in the 3x3 residual convolutions)");
    if (o.i("load_probe") > 0 && y4m_in) die("-load_probe probes the file loaders: it cannot be combined with -input_y4m");
    if (o.i("load_probe") > 0) {
        favp::Poll poll; poll.timeout_s = o.d("poll_timeout"); poll.settle_s = std::max(0.0, o.d("poll_settle")); poll.out = favl::msg();
        const auto t0 = std::chrono::steady_clock::now();
        FrameIn in = load_frame_inputs(o, poll, o.i("load_probe"), false, nullptr, 0);
        auto fnv = [](const void* p, size_t n) { unsigned long long h = 1469598103934665603ull; const uint8_t* b = (const uint8_t*)p;
                                                 if (!p) return 0ull; for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; } return h; };
        const size_t n = (size_t)in.W * in.H;
        size_t cert255 = 0; if (in.cert) for (size_t i = 0; i < n; ++i) cert255 += in.cert[i] == 255;
        fprintf(favl::msg(), "{\"ok\": %s, \"W\": %d, \"H\": %d, \"seconds\": %.3f, \"frame\": \"%016llx\", \"cert\": \"%016llx\", \"cert_255\": %zu, \"bw\": \"%016llx\", \"fw\": \"%016llx\"}\n",
               in.ok ? "true" : "false", in.W, in.H, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(),
               fnv(in.frame, n * 3), fnv(in.cert, n), cert255, fnv(in.bw, n * 8), fnv(in.fw, n * 8));
        return in.ok ? 0 : 1;
    }
    const bool dry = o.i("dry_run") != 0;
    std::vector<std::string> streams = favl::split_list(o.s("streams"));
    const bool named = !streams.empty();
    if (!named) streams.push_back("");
    int world = std::max(1, o.i("gpus"));
    const int rank = o.i("worker_rank");
    static const char* const path_opts[] = {"input_pattern", "flow_pattern", "forward_flow_pattern", "occlusions_pattern", "output_prefix", "temporal_eval_file",
                                            "input_y4m", "output_y4m"};
    if (named && streams.size() > 1 && o.s(y4m_out ? "output_y4m" : "output_prefix").find("%S") == std::string::npos)
        die(std::string("-streams: -") + (y4m_out ? "output_y4m" : "output_prefix") + " must contain %S (the streams would overwrite each other's frames)");
    if (named && streams.size() > 1 && !o.s("scene_cut_log").empty() && o.s("scene_cut_log").find("%S") == std::string::npos)
        die("-streams: -scene_cut_log must contain %S (the streams would overwrite each other's log)");

    // ------------------------------------------------------------------------------------------ launcher
    if (rank < 0 && (world > 1 || o.i("force_dist"))) {
        if (!dry) {
            std::vector<std::string> models{o.s("model_vid")};
            if (o.s("model_img") != "self") models.push_back(o.s("model_img"));
            favl::validate_models(models);                        // before any worker exists: ERROR + nonzero exit, never a hang
            const int ndev = fav_device_count();
            if (ndev <= 0) die(std::string("ERROR: ") + fav_last_error());
            if (o.i("gpu") + world > ndev) die("-gpus " + o.s("gpus") + " from -gpu " + o.s("gpu") + ": only " + std::to_string(ndev) + " devices");
        }
        if (dry)      // what the host can sustain at most, whatever the GPUs do (the 8-GPU run explains itself)
            fprintf(favl::msg(), "{\"host_ceiling\": %s}\n", favl::host_ceiling_json(o.s("png_encoder") == "gpu" ? favl::HOST_CPU_MS_PER_FRAME_GPU_PNG : favl::HOST_CPU_MS_PER_FRAME_HOST_PNG,
                                                                       "default: measured on the project's MI355X box at 1280x720, fused 3-argument check").c_str());
        std::string xdir;
        const int worst = favl::spawn_workers(argc, argv, world, o.i("pin_workers") != 0, &xdir);
        if (o.i("timing") && !dry && worst == 0) favl::print_aggregate(xdir, world, streams.size());
        favl::remove_exchange_dir(xdir, world);
        return worst;
    }

    // ------------------------------------------------------------------------------------------ worker / single process
    const bool dist = rank >= 0;
    if (dist) world = o.i("worker_world");
    const int device = o.i("gpu") + (dist ? rank : 0);
    std::vector<std::string> mine;
    for (size_t s = 0; s < streams.size(); ++s) if (!dist || (int)(s % (size_t)world) == rank) mine.push_back(streams[s]);     // stream s -> GPU s mod N
    const int nwriters = favl::writer_budget(o.i("writers"), dist ? world : 1, dist && world > 1 && o.i("pin_workers") != 0);
    if (dry) {
        favl::dry_run_failure_hook(rank);
        std::string js = "{\"rank\": " + std::to_string(std::max(rank, 0)) + ", \"world\": " + std::to_string(dist ? world : 1) + ", \"device\": " + std::to_string(device) +
                         ", \"cpus\": " + std::to_string(favl::allowed_cpus().size()) + ", \"writers\": " + std::to_string(nwriters) + ", \"streams\": [";
        for (size_t k = 0; k < mine.size(); ++k) {
            js += std::string(k ? ", " : "") + "{\"name\": " + favl::json_str(mine[k]);
            for (const char* po : path_opts) js += std::string(", \"") + po + "\": " + favl::json_str(named ? favl::subst_stream(o.s(po), mine[k]) : o.s(po));
            // the output stream's C tag; with a Y4M input and neither format option it is the input's, which only its header says
            if (y4m_out) js += ", \"output_y4m_tag\": " + favl::json_str(y4m_in && o.s("y4m_format").empty() && o.s("y4m_pixel_format").empty()
                                                                            ? std::string("input") : y4m_tag_of(y4m_layout_of(o, nullptr, 0, true)));
            js += "}";
        }
        fprintf(favl::msg(), "%s]}\n", js.c_str());
        return 0;
    }

    if (fav_device_count() <= 0) die(std::string("ERROR: ") + fav_last_error());
    if (hipSetDevice(device) != hipSuccess) die("cannot select GPU " + std::to_string(device));
    const bool want_img = o.s("model_img") != "self";
    fav_net* net = nullptr; fav_net* net_img = nullptr;                                                      // core.lua:39-66
    favl::DistTimes dist_times;
    if (dist) {
        // rank 0 parses; the other ranks never open the .t7
        favl::load_models_dist(rank, world, o.s("rccl_id_file"), device, o.s("model_vid"), want_img ? o.s("model_img") : std::string(), &net, &net_img,
                               mine.size(), nwriters, &dist_times);
    } else {
        if (fav_net_create(o.s("model_vid").c_str(), device, &net)) die(fav_last_error());                   // core.lua:39-43
        if (want_img && fav_net_create(o.s("model_img").c_str(), device, &net_img)) die(fav_last_error());
    }
    check(fav_net_set_precision(net, o.s("precision") == "bf16" ? FAV_PRECISION_BF16_OPERANDS : FAV_PRECISION_FP32), "fav_net_set_precision");
    if (o.i("shared_gpu")) { check(fav_net_set_shared_device(net, 1), "fav_net_set_shared_device"); if (net_img) check(fav_net_set_shared_device(net_img, 1), "fav_net_set_shared_device"); }
    fprintf(favl::msg(), "Model loaded.\n");
    if (net_img) fprintf(favl::msg(), "Model loaded.\n");

    int frames = 0; double seconds = 0, cpu_seconds = 0;
    for (const std::string& name : mine) {
        Opt os = o;
        if (named) for (const char* po : path_opts) os.v[po] = favl::subst_stream(o.s(po), name);
        if (named) os.v["scene_cut_log"] = favl::subst_stream(o.s("scene_cut_log"), name);
        StreamResult r;
        StreamRun(os, flow_opts, net, net_img, nwriters).run(&r);
        frames += r.frames; seconds += r.seconds; cpu_seconds += r.cpu_s;
        if (o.i("timing"))
            fprintf(favl::msg(), "{%s\"frames\": %d, \"seconds\": %.4f, \"fps_end_to_end\": %.3f, \"wait_loader_s\": %.3f, \"h2d_gpu_d2h_s\": %.3f, \"wait_png_pool_s\": %.3f, \"setup_s\": %.3f, \"png_tail_s\": %.3f, \"png_writers\": %d, "
                   "\"png_encoder\": \"%s\", \"host_cpu_ms_per_frame\": %.3f, \"cpu_ms_per_frame_loaders\": %.3f, \"cpu_ms_per_frame_writers\": %.3f, \"cpu_ms_per_frame_writers_waiting_for_the_copy\": %.3f, \"cpu_ms_per_frame_main\": %.3f, "
                   "\"png_mb_per_frame\": %.3f, \"usable_cpus\": %d}\n",
                   named ? ("\"stream\": " + favl::json_str(name) + ", \"gpu\": " + std::to_string(device) + ", ").c_str() : "",
                   r.frames, r.seconds, r.frames / std::max(r.seconds, 1e-9), r.wait_loader, r.wait_gpu, r.wait_png, r.setup, r.tail, nwriters,
                   o.s("png_encoder").c_str(), 1e3 * r.cpu_s / std::max(r.frames, 1), 1e3 * r.cpu_loaders / std::max(r.frames, 1), 1e3 * r.cpu_writers / std::max(r.frames, 1), 1e3 * r.cpu_writer_sync / std::max(r.frames, 1),
                   1e3 * r.cpu_main / std::max(r.frames, 1), 1e-6 * (double)r.png_bytes / std::max(r.frames, 1), favl::effective_cpus());
    }
    check(fav_net_check(net), "at exit");
    if (net_img) check(fav_net_check(net_img), "at exit (image model)");
    if (o.i("timing")) fprintf(favl::msg(), "thread CPU seconds (live threads, whole process): %s\n", thread_cpu_report().c_str());
    if (dist && o.i("timing")) favl::write_worker_result(o.s("rccl_id_file"), rank, frames, seconds, cpu_seconds, dist_times);
    fflush(favl::msg());
    fav_net_destroy(net); fav_net_destroy(net_img);
    return 0;
}
