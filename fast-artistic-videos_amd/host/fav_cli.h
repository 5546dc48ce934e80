// fav_cli.h -- what the host programs share: the fatal-error convention (die: message on stderr, exit 1), the file-name patterns of the
// reference's CLIs, polled reads, strict integers, owning handles (csrc/dev_handles.h) filled the programs' way -- a failure is fatal --
// and the -flow_* flags of the built-in estimator (fav_stylize, fav_stylize_vr).
#pragma once
#include <hip/hip_runtime.h>
#include <sys/stat.h>

#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>

#include "../../include/fav.h"
#include "../csrc/dev_handles.h"
#include "fav_poll.h"

namespace favl {

[[noreturn]] inline void die(const std::string& m) { fprintf(stderr, "%s\n", m.c_str()); exit(1); }
// where the messages go: stdout, unless the caller's stdout carries data (fav_stylize -output_y4m -)
inline FILE*& msg() { static FILE* f = stdout; return f; }

inline void check(int rc, const char* what) { if (rc) die(std::string(what) + ": " + fav_last_error()); }

inline bool file_exists(const std::string& p) { struct stat st; return stat(p.c_str(), &st) == 0 && S_ISREG(st.st_mode); }

inline void mkdirs_for(const std::string& path)
{
    for (size_t p = 1; p < path.size(); ++p)
        if (path[p] == '/') mkdir(path.substr(0, p).c_str(), 0777);
}

inline std::string fmt_int(const std::string& pattern, int i) { char b[4096]; snprintf(b, sizeof b, pattern.c_str(), i); return b; }
inline std::string fmt_int(const std::string& pattern, int i, int j) { char b[4096]; snprintf(b, sizeof b, pattern.c_str(), i, j); return b; }

// getFormatedFlowFileName (fast_artistic_video.lua:70-77): {fmt} <- fromIndex, [fmt] <- toIndex;
// face >= 0 (fast_artistic_video_vr.lua:105-115): then the remaining %d <- face id
inline std::string flow_name(const std::string& pattern, int from, int to, int face = -1)
{
    std::string out;
    for (size_t p = 0; p < pattern.size();) {
        const char c = pattern[p];
        if (c == '{' || c == '[') {
            const size_t e = pattern.find(c == '{' ? '}' : ']', p + 1);
            if (e != std::string::npos) { out += fmt_int(pattern.substr(p + 1, e - p - 1), c == '{' ? from : to); p = e + 1; continue; }
        }
        out += c; ++p;
    }
    return face >= 0 ? fmt_int(out, face) : out;
}

// utils.wait_for_file (fast_artistic_video/utils.lua:74-80) with the settle rule of fav_poll.h: wait, read, and poll again while the
// file reads short under a producer that is still writing it.  `what` names the read in the message of a reader that fails.
template <class Reader>
void read_polled(const std::string& path, const favp::Poll& p, const char* what, Reader&& reader)
{
    bool timed_out = false;
    const int rc = favp::read_when_complete(path, p, reader, &timed_out);
    if (timed_out) die("timed out waiting for " + path);
    check(rc, what);
}

// a whole decimal number of at most seven digits, nothing before or after it
inline bool parse_int(const char* s, int* out)
{
    char* end = nullptr;
    const long v = strtol(s, &end, 10);
    if (end == s || *end != '\0' || v < -1000000 || v > 1000000) return false;
    *out = (int)v;
    return true;
}

// ---- handles, filled or fatal -------------------------------------------------------------------------------------------------
// what == null: "<call> failed"; otherwise "<what>: <the runtime's error text>" (fav_stylize_vr's wording)
inline void hip_or_die(hipError_t e, const char* call, const char* what)
{
    if (e != hipSuccess) die(what ? std::string(what) + ": " + hipGetErrorString(e) : std::string(call) + " failed");
}

template <class T> fav::dev_ptr<T> dev_alloc(size_t bytes, const char* what = nullptr)
{
    void* p = nullptr; hip_or_die(hipMalloc(&p, bytes), "hipMalloc", what);
    return fav::dev_ptr<T>(static_cast<T*>(p));
}

template <class T> fav::host_ptr<T> host_alloc(size_t bytes, const char* what = nullptr)
{
    void* p = nullptr; hip_or_die(hipHostMalloc(&p, bytes, hipHostMallocDefault), "hipHostMalloc", what);
    return fav::host_ptr<T>(static_cast<T*>(p));
}

inline fav::event_h event_create(unsigned flags)
{
    hipEvent_t e = nullptr; hip_or_die(hipEventCreateWithFlags(&e, flags), "hipEventCreate", nullptr);
    return fav::event_h(e);
}

// a BLOCKING queue, as the programs have always used (csrc/dev_owned.h's is non-blocking); the handle drains it before it goes
inline fav::queue_h queue_create(const char* what = nullptr)
{
    hipStream_t q = nullptr; hip_or_die(hipStreamCreate(&q), "hipStreamCreate", what);
    return fav::queue_h(q);
}

// ---- the estimator's flags ----------------------------------------------------------------------------------------------------
using Flags = std::map<std::string, std::string>;

// the -flow_* flags fav_stylize and fav_stylize_vr share, each with the default 0 (fav_flow_opts*: 0 = the estimator's default / off);
// fav_stylize has -flow_levels besides
inline void add_flow_flags(Flags& v)
{
    for (const char* k : {"flow_alpha", "flow_eps", "flow_grad", "flow_match", "flow_median", "flow_iters", "flow_warps"}) v[k] = "0";
}

// the switches among them: a value outside the set is refused, and so is one that is on while the estimator is not -- `needs` names
// what turns the estimator on ("-estimate_flow 1", "-input_equi_pattern")
inline void validate_flow_flags(const Flags& v, bool estimator_on, const char* needs)
{
    const std::string &g = v.at("flow_grad"), &m = v.at("flow_match"), &d = v.at("flow_median");
    if (g != "0" && g != "1") die("-flow_grad must be 0 or 1, not '" + g + "'");
    if (g == "1" && !estimator_on) die(std::string("-flow_grad 1 selects the data term of the built-in flow estimator: it needs ") + needs);
    if (m != "0" && m != "1") die("-flow_match must be 0 or 1, not '" + m + "'");
    if (m == "1" && !estimator_on) die(std::string("-flow_match 1 turns on the matching prior of the built-in flow estimator: it needs ") + needs);
    if (d != "0" && d != "3" && d != "5") die("-flow_median must be 0, 3 or 5, not '" + d + "'");
    if (d != "0" && !estimator_on) die("-flow_median " + d + " turns on the median filter of the built-in flow estimator: it needs " + needs);
}

// the estimator's options from the flags (validated above; a program without -flow_levels gets the default pyramid)
inline fav_flow_opts_ex3 flow_opts_of(const Flags& v)
{
    auto s = [&](const char* k) { const auto it = v.find(k); return it == v.end() ? "0" : it->second.c_str(); };
    return {{{{atoi(s("flow_levels")), atoi(s("flow_warps")), atoi(s("flow_iters")), (float)atof(s("flow_alpha")), 0, (float)atof(s("flow_eps"))}, atoi(s("flow_grad"))},
             atoi(s("flow_match")) ? -1.f : 0.f, 0},
            atoi(s("flow_median"))};
}

}  // namespace favl
