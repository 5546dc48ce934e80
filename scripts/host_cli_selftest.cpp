// host_cli_selftest -- the parts of the host programs' shared header (host/fav_cli.h) and of the Y4M plumbing (host/fav_y4m.h) that
// need no GPU, as one stand-alone program for a sanitizer build on the CPU:
//   cd fast-artistic-videos_amd && hipcc -std=c++17 -x hip --offload-arch=gfx950 -O1 -g -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=undefined ../scripts/host_cli_selftest.cpp -o /tmp/host_cli_selftest -L. -lfav -Wl,-rpath,$PWD
//   /tmp/host_cli_selftest            (prints "host_cli_selftest: N checks passed", exit 0)
// No device is touched: nothing here calls the HIP runtime.  A flag combination that must be refused runs in a child process (die()
// exits), whose stderr and exit status are the result.
#include <sys/wait.h>
#include <unistd.h>

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../fast-artistic-videos_amd/host/fav_cli.h"
#include "../fast-artistic-videos_amd/host/fav_y4m.h"

namespace {

int checks = 0;
void expect(bool ok, const std::string& what)
{
    ++checks;
    if (!ok) { fprintf(stderr, "host_cli_selftest: FAILED: %s\n", what.c_str()); exit(1); }
}

// validate_flow_flags in a child: exit status and first line of stderr
std::pair<int, std::string> validate(const favl::Flags& v, bool on, const char* needs)
{
    int pp[2];
    if (pipe(pp)) { perror("pipe"); exit(1); }
    fflush(stdout); fflush(stderr);
    const pid_t pid = fork();
    if (pid == 0) { dup2(pp[1], 2); close(pp[0]); close(pp[1]); favl::validate_flow_flags(v, on, needs); _exit(0); }
    close(pp[1]);
    std::string err; char buf[512]; ssize_t n;
    while ((n = read(pp[0], buf, sizeof buf)) > 0) err.append(buf, (size_t)n);
    close(pp[0]);
    int st = 0; waitpid(pid, &st, 0);
    return {WIFEXITED(st) ? WEXITSTATUS(st) : -1, err.substr(0, err.find('\n'))};
}

void flow_flags()
{
    favl::Flags base; favl::add_flow_flags(base);
    expect(base.size() == 7 && base.at("flow_median") == "0" && !base.count("flow_levels"), "seven shared flags, each 0");
    const char* const values[] = {"0", "1", "2", "3", "5", "", "x", "-1", "01", "1 ", "3.0"};
    struct Sw { const char* name; std::vector<std::string> legal; const char* must; const char* on_text; };
    const Sw sws[] = {{"flow_grad", {"0", "1"}, "-flow_grad must be 0 or 1, not '", "-flow_grad 1 selects the data term of the built-in flow estimator: it needs "},
                      {"flow_match", {"0", "1"}, "-flow_match must be 0 or 1, not '", "-flow_match 1 turns on the matching prior of the built-in flow estimator: it needs "},
                      {"flow_median", {"0", "3", "5"}, "-flow_median must be 0, 3 or 5, not '", nullptr}};
    for (const char* needs : {"-estimate_flow 1", "-input_equi_pattern"})
        for (const Sw& sw : sws)
            for (const char* val : values)
                for (bool on : {false, true}) {
                    favl::Flags v = base; v[sw.name] = val;
                    const auto r = validate(v, on, needs);
                    bool legal = false; for (const auto& l : sw.legal) legal |= l == val;
                    const std::string what = std::string("-") + sw.name + " '" + val + "' estimator " + (on ? "on" : "off") + ": " + r.second;
                    if (!legal) expect(r.first == 1 && r.second == std::string(sw.must) + val + "'", what);
                    else if (on || !strcmp(val, "0")) expect(r.first == 0 && r.second.empty(), what);
                    else if (sw.on_text) expect(r.first == 1 && r.second == std::string(sw.on_text) + needs, what);
                    else expect(r.first == 1 && r.second == std::string("-flow_median ") + val + " turns on the median filter of the built-in flow estimator: it needs " + needs, what);
                }
    favl::Flags v = base;
    v["flow_alpha"] = "12.5"; v["flow_eps"] = "0.3"; v["flow_iters"] = "7"; v["flow_warps"] = "3"; v["flow_grad"] = "1"; v["flow_match"] = "1"; v["flow_median"] = "5";
    fav_flow_opts_ex3 o = favl::flow_opts_of(v);
    expect(o.median == 5 && o.ex2.match_beta == -1.f && o.ex2.match_radius == 0 && o.ex2.ex.data_term == 1 && o.ex2.ex.base.levels == 0 && o.ex2.ex.base.warps == 3 &&
           o.ex2.ex.base.iters == 7 && o.ex2.ex.base.alpha == 12.5f && o.ex2.ex.base.smooth_eps == 0.3f, "flow_opts_of without -flow_levels");
    v["flow_levels"] = "4"; v["flow_match"] = "0";
    o = favl::flow_opts_of(v);
    expect(o.ex2.ex.base.levels == 4 && o.ex2.match_beta == 0.f, "flow_opts_of with -flow_levels");
}

void names_and_numbers()
{
    using favl::flow_name;
    expect(flow_name("flow/backward_[%d]_{%d}.flo", 3, 4) == "flow/backward_4_3.flo", "flow_name [to] {from}");
    expect(flow_name("f_{%05d}_[%03d]", 7, 8) == "f_00007_008", "flow_name with widths");
    expect(flow_name("flow_768-%d/backward_[%d]_{%d}.flo", 1, 2, 6) == "flow_768-6/backward_2_1.flo", "flow_name with a face");
    expect(flow_name("plain.flo", 1, 2) == "plain.flo" && flow_name("", 1, 2).empty(), "flow_name without tokens");
    expect(flow_name("open_{%d", 1, 2) == "open_{%d" && flow_name("x]_[%d]", 1, 2) == "x]_2", "flow_name with unbalanced brackets");
    expect(flow_name(std::string(5000, 'a') + "{%d}", 1, 2).size() == 5001, "flow_name of a long pattern");
    expect(favl::fmt_int("frame_%05d.ppm", 12) == "frame_00012.ppm" && favl::fmt_int("frame_%05d-%d.ppm", 12, 6) == "frame_00012-6.ppm", "fmt_int");
    int x = 99;
    for (const char* good : {"0", "-1", "1000000", "-1000000", "007", "+5"}) expect(favl::parse_int(good, &x), std::string("parse_int accepts ") + good);
    expect(favl::parse_int("-1000000", &x) && x == -1000000, "parse_int value");
    x = 99;
    for (const char* bad : {"", " ", "1 ", "1x", "x", "1.0", "1000001", "-1000001", "99999999999999999999", "0x10"})
        expect(!favl::parse_int(bad, &x) && x == 99, std::string("parse_int refuses '") + bad + "'");
    expect(!favl::file_exists("/") && !favl::file_exists("/nonexistent/file"), "file_exists wants a regular file");
}

void y4m_header()
{
    char path[] = "/tmp/host_cli_selftest_XXXXXX";
    const int fd = mkstemp(path);
    expect(fd >= 0, "mkstemp"); close(fd);
    fav_y4m_header h; memset(&h, 0, sizeof h);
    h.W = 34; h.H = 18; h.fps_num = 30000; h.fps_den = 1001; h.interlace = 'p'; h.aspect_num = h.aspect_den = 1;
    h.fmt = fav_yuv_format{FAV_YUV_420, FAV_YUV_SITING_CENTER, FAV_YUV_BT601, 1};
    const size_t bytes = fav_yuv_frame_bytes(h.W, h.H, &h.fmt);
    expect(bytes == 34u * 18u + 2u * 17u * 9u, "4:2:0 frame bytes");
    std::vector<uint8_t> planes(bytes);
    for (size_t i = 0; i < bytes; ++i) planes[i] = (uint8_t)(i * 7);
    {
        favy::Writer w;
        expect(w.open(path) && w.header(h) && w.frame(planes.data(), bytes) && w.frame(planes.data(), bytes), "Y4M written");
        expect(favy::write_full(1, "", 0), "write_full of nothing");
    }
    {
        favy::Reader r;
        expect(r.open(path).empty(), "Y4M header read back");
        const fav_y4m_header& g = r.header();
        expect(g.W == h.W && g.H == h.H && g.fps_num == h.fps_num && g.fps_den == h.fps_den && g.interlace == 'p' && g.fmt.chroma == FAV_YUV_420 && g.fmt.full_range == 1, "Y4M header fields");
        r.set_frame_bytes(bytes);
        std::vector<uint8_t> got(bytes);
        expect(r.read_frame(1, got.data()) == favy::Reader::FRAME && got == planes, "frame 1");
        expect(r.read_frame(2, got.data()) == favy::Reader::FRAME && got == planes, "frame 2");
        expect(r.read_frame(3, got.data()) == favy::Reader::END && r.read_frame(4, got.data()) == favy::Reader::END && r.failed_at() == 0, "the stream ends at a frame boundary");
    }
    char hb[FAV_Y4M_MAX_HEADER + 1];
    const int hn = fav_y4m_format_header_host(&h, hb, sizeof hb);
    expect(hn > 0 && truncate(path, (off_t)(hn + 6 + bytes + 6 + 10)) == 0, "truncate inside frame 2");
    {
        favy::Reader r;
        expect(r.open(path).empty(), "truncated stream opens");
        r.set_frame_bytes(bytes);
        std::vector<uint8_t> got(bytes);
        expect(r.read_frame(1, got.data()) == favy::Reader::FRAME, "frame 1 of the truncated stream");
        expect(r.read_frame(2, got.data()) == favy::Reader::TRUNCATED && r.failed_at() == 2 && r.failure() == favy::Reader::TRUNCATED, "the stream ends inside frame 2");
    }
    expect(truncate(path, 5) == 0, "truncate into the header");
    { favy::Reader r; expect(r.open(path) == std::string(path) + ": the stream ends inside its header", "a header cut short"); }
    { favy::Reader r; expect(r.open("/nonexistent/in.y4m") == "Could not open /nonexistent/in.y4m", "a missing stream"); }
    unlink(path);
}

}  // namespace

int main()
{
    flow_flags();
    names_and_numbers();
    y4m_header();
    printf("host_cli_selftest: %d checks passed\n", checks);
    return 0;
}
