// fav_flow -- drop-in for the reference's `run-deepflow.sh <img1> <img2> <out.flo> [downscale]` (makeOptFlow_deepflow.sh:46-49), which
// needs two closed CPU binaries: the flow from img1 to img2 (img2(p + w(p)) ~ img1(p)) with libfav's variational estimator
// (fav_flow_rgb8: Horn-Schunck with warping, coarse to fine -- no descriptor matching; DESIGN.md, "fav_flow").
//
//   fav_flow [options] <img1.ppm> <img2.ppm> <out.flo> [downscale]      the 4th argument is accepted and ignored
//   fav_flow [options] -batch <list.txt>                                one "img1 img2 out.flo" per line: start-up is paid once
//   options: -alpha <x>  -iters <n>  -warps <n>  -levels <n>  (0 = default, each)   -gpu <n>
//            -eps <x>    edge-preserving smoothness (fav_flow_opts.smooth_eps; 0 = off, the default; 0.3 is the measured choice)
//            -grad <0|1> data term on the image gradients instead of the grey levels (fav_flow_opts_ex.data_term; 0 = off, the default):
//                        for frames whose lighting changes
//            -match <0|1> block-matching prior for objects that move further than their own size (fav_flow_opts_ex2.match_beta: the
//                        default weight; 0 = off, the default);  -match_radius <n>  its search radius at half resolution (1..32; 0 = 16)
//            -median <0|3|5> median filtering of the flow after every warp, the side of the window (fav_flow_opts_ex3.median; 0 = off,
//                        the default)
//
// The .flo is written under a temporary name and renamed into place, so a polling consumer never reads a partial file.
#include <hip/hip_runtime.h>
#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/fav.h"
#include "fav_cli.h"

namespace {

using favl::die; using favl::parse_int;

[[noreturn]] void usage(const std::string& why)
{
    fprintf(stderr, "%s\nusage: fav_flow [-alpha x] [-eps x] [-grad 0|1] [-match 0|1] [-match_radius n] [-median 0|3|5] [-iters n] [-warps n] [-levels n] [-gpu n] <img1.ppm> <img2.ppm> <out.flo> [downscale]\n"
                    "       fav_flow [options] -batch <list.txt>      (one \"img1 img2 out.flo\" per line)\n", why.c_str());
    exit(2);
}

struct Job { std::string a, b, out; };

bool write_flo(const std::string& path, const float* uv, int W, int H)
{
    const std::string tmp = path + ".tmp." + std::to_string((long long)getpid());
    FILE* f = fopen(tmp.c_str(), "wb");
    if (!f) return false;
    const float tag = 202021.25f;      // "PIEH"
    const size_t n = (size_t)W * H * 2;
    const bool ok = fwrite(&tag, 4, 1, f) == 1 && fwrite(&W, 4, 1, f) == 1 && fwrite(&H, 4, 1, f) == 1 && fwrite(uv, 4, n, f) == n;
    if (fclose(f) != 0 || !ok || rename(tmp.c_str(), path.c_str()) != 0) { unlink(tmp.c_str()); return false; }
    return true;
}

}  // namespace

int main(int argc, char** argv)
{
    fav_flow_opts_ex3 fx3 = {};    // every field 0: the defaults, the brightness term, no matching prior, no median filter
    fav_flow_opts_ex2& fx2 = fx3.ex2;
    fav_flow_opts_ex& fx = fx2.ex;
    fav_flow_opts& fo = fx.base;
    int gpu = 0;
    std::string batch;
    std::vector<std::string> pos;
    for (int a = 1; a < argc; ++a) {
        const std::string k = argv[a];
        if (k.size() > 1 && k[0] == '-' && !(k[1] >= '0' && k[1] <= '9') && k[1] != '.') {
            if (a + 1 >= argc) usage("missing value for " + k);
            const char* v = argv[++a];
            bool ok = true;
            if (k == "-batch") batch = v;
            else if (k == "-alpha") { char* end = nullptr; fo.alpha = strtof(v, &end); ok = end != v && *end == '\0'; }
            else if (k == "-eps") { char* end = nullptr; fo.smooth_eps = strtof(v, &end); ok = end != v && *end == '\0'; }
            else if (k == "-grad") { if (strcmp(v, "0") != 0 && strcmp(v, "1") != 0) usage(std::string("-grad must be 0 or 1, not '") + v + "'"); fx.data_term = v[0] - '0'; }
            else if (k == "-match") { if (strcmp(v, "0") != 0 && strcmp(v, "1") != 0) usage(std::string("-match must be 0 or 1, not '") + v + "'"); fx2.match_beta = v[0] == '1' ? -1.f : 0.f; }
            else if (k == "-match_radius") ok = parse_int(v, &fx2.match_radius);
            else if (k == "-median") { if (strcmp(v, "0") != 0 && strcmp(v, "3") != 0 && strcmp(v, "5") != 0) usage(std::string("-median must be 0, 3 or 5, not '") + v + "'"); fx3.median = v[0] - '0'; }
            else if (k == "-iters") ok = parse_int(v, &fo.iters);
            else if (k == "-warps") ok = parse_int(v, &fo.warps);
            else if (k == "-levels") ok = parse_int(v, &fo.levels);
            else if (k == "-gpu") ok = parse_int(v, &gpu) && gpu >= 0;
            else usage("unknown option " + k);
            if (!ok) usage("bad value for " + k + ": '" + v + "'");
        } else pos.push_back(k);
    }
    std::vector<Job> jobs;
    if (!batch.empty()) {
        if (!pos.empty()) usage("-batch takes its file names from the list, not from the command line");
        std::ifstream in(batch);
        if (!in) die("Could not open " + batch);
        std::string line; int ln = 0;
        while (std::getline(in, line)) {
            ++ln;
            std::istringstream ss(line);
            Job j; std::string extra;
            if (!(ss >> j.a)) continue;                  // empty line
            if (!(ss >> j.b >> j.out) || (ss >> extra)) die(batch + ":" + std::to_string(ln) + ": expected \"img1 img2 out.flo\"");
            jobs.push_back(j);
        }
    } else {
        if (pos.size() < 3 || pos.size() > 4) usage("expected <img1.ppm> <img2.ppm> <out.flo> [downscale]");
        jobs.push_back({pos[0], pos[1], pos[2]});        // pos[3]: run-deepflow.sh's downscale factor, of no use here
    }
    if (fav_flow_workspace_bytes_ex3(64, 64, &fx3) == 0) die(fav_last_error());      // the options, before any file or device is touched

    if (fav_device_count() <= 0) die(std::string("ERROR: ") + fav_last_error());
    if (hipSetDevice(gpu) != hipSuccess) die("cannot select GPU " + std::to_string(gpu));
    fav::dev_ptr<uint8_t> d_a, d_b; fav::dev_ptr<float> d_flow; fav::dev_ptr<void> d_ws;
    int cw = 0, ch = 0; size_t ws_bytes = 0;
    std::vector<float> h_flow;
    for (const Job& j : jobs) {
        uint8_t *a = nullptr, *b = nullptr; int W, H, W2, H2, c1, c2;
        if (fav_read_pnm_host(j.a.c_str(), &a, &W, &H, &c1)) die(fav_last_error());
        if (fav_read_pnm_host(j.b.c_str(), &b, &W2, &H2, &c2)) die(fav_last_error());
        if (c1 != 3 || c2 != 3) die(j.a + ", " + j.b + ": expected colour (P6) frames");
        if (W != W2 || H != H2) die(j.a + ", " + j.b + ": the two frames differ in size");
        const size_t n = (size_t)W * H;
        if (W != cw || H != ch) {
            ws_bytes = fav_flow_workspace_bytes_ex3(W, H, &fx3);
            if (!ws_bytes) die(fav_last_error());
            d_a.reset(); d_b.reset(); d_flow.reset(); d_ws.reset();      // the old size goes before the new one comes
            d_a = favl::dev_alloc<uint8_t>(n * 3); d_b = favl::dev_alloc<uint8_t>(n * 3); d_flow = favl::dev_alloc<float>(n * 8); d_ws = favl::dev_alloc<void>(ws_bytes);
            h_flow.resize(n * 2); cw = W; ch = H;
        }
        if (hipMemcpy(d_a.get(), a, n * 3, hipMemcpyHostToDevice) || hipMemcpy(d_b.get(), b, n * 3, hipMemcpyHostToDevice)) die("upload failed");
        fav_free_host(a); fav_free_host(b);
        if (fav_flow_rgb8_ex3(d_a.get(), d_b.get(), W, H, &fx3, d_flow.get(), d_ws.get(), ws_bytes, nullptr)) die(fav_last_error());
        if (hipMemcpy(h_flow.data(), d_flow.get(), n * 8, hipMemcpyDeviceToHost) != hipSuccess) die("GPU error while estimating " + j.out);
        if (!write_flo(j.out, h_flow.data(), W, H)) die("cannot write " + j.out);
    }
    return 0;
}
