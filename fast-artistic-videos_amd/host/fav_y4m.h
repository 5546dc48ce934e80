// fav_y4m.h -- the YUV4MPEG2 streams of fav_stylize (-input_y4m / -output_y4m): a sequential reader that several loader threads may
// share, and a writer.  The header grammar is libfav's (fav_y4m_parse_stream_header_host / fav_y4m_format_stream_header_host,
// include/fav_yuv.h: every layout); this file only moves bytes: `YUV4MPEG2 ...\n`, then per frame `FRAME[ params]\n` and
// fav_yuv_layout_frame_bytes bytes.  PATH `-` is stdin / stdout.
#pragma once
#include <fcntl.h>
#include <unistd.h>

#include <cerrno>
#include <condition_variable>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <string>

#include "../../include/fav.h"

namespace favy {

// exactly n bytes unless the stream ends first (a pipe hands over what it has: short reads are the rule); -1: read error
inline ssize_t read_full(int fd, void* buf, size_t n)
{
    size_t got = 0;
    while (got < n) {
        const ssize_t k = read(fd, static_cast<char*>(buf) + got, n - got);
        if (k < 0) { if (errno == EINTR) continue; return -1; }
        if (k == 0) break;
        got += (size_t)k;
    }
    return (ssize_t)got;
}

inline bool write_full(int fd, const void* buf, size_t n)
{
    size_t put = 0;
    while (put < n) {
        const ssize_t k = write(fd, static_cast<const char*>(buf) + put, n - put);
        if (k < 0) { if (errno == EINTR) continue; return false; }
        put += (size_t)k;
    }
    return true;
}

class Reader {
public:
    enum Status { FRAME, END, TRUNCATED, BAD };
    ~Reader() { if (fd_ > 0) close(fd_); }
    // opens the stream and parses its header; "" or what went wrong
    std::string open(const std::string& path)
    {
        fd_ = path == "-" ? 0 : ::open(path.c_str(), O_RDONLY);
        if (fd_ < 0) return "Could not open " + path;
        char line[FAV_Y4M_MAX_HEADER + 1];
        size_t n = 0;
        for (; n < sizeof line; ++n) {
            const ssize_t k = read_full(fd_, line + n, 1);
            if (k < 0) return path + ": read error";
            if (k == 0) return path + ": the stream ends inside its header";
            if (line[n] == '\n') break;
        }
        if (fav_y4m_parse_stream_header_host(line, n, &hdr_)) return path + ": " + fav_last_error();
        return "";
    }
    const fav_y4m_stream_header& header() const { return hdr_; }
    void set_frame_bytes(size_t n) { frame_bytes_ = n; }
    // Frame `index` (1, 2, ...) into dst.  Callers on several threads each wait for their turn, so the indices must be asked for without
    // gaps.  END: the stream ended at a frame boundary (also for every later index); TRUNCATED: it ended inside this frame.
    Status read_frame(int index, uint8_t* dst)
    {
        std::unique_lock<std::mutex> l(m_);
        turn_.wait(l, [&] { return ended_ || next_ == index; });
        if (ended_) return END;
        Status st = FRAME;
        char tag[6];
        const ssize_t k = read_full(fd_, tag, 6);
        if (k == 0) st = END;
        else if (k < 0) st = BAD;
        else if (k < 6) st = TRUNCATED;
        else if (memcmp(tag, "FRAME", 5) || (tag[5] != '\n' && tag[5] != ' ')) st = BAD;
        for (char c = st == FRAME ? tag[5] : '\n'; c != '\n';) {             // parameters of the frame: skipped
            const ssize_t g = read_full(fd_, &c, 1);
            if (g <= 0) { st = g < 0 ? BAD : TRUNCATED; break; }
        }
        if (st == FRAME) {
            const ssize_t g = read_full(fd_, dst, frame_bytes_);
            if (g < 0) st = BAD; else if ((size_t)g < frame_bytes_) st = TRUNCATED;
        }
        if (st == FRAME) ++next_;
        else { ended_ = true; if (st != END) { failed_at_ = index; failure_ = st; } }
        l.unlock();
        turn_.notify_all();
        return st;
    }
    // the frame inside which the stream ended or was damaged (0: none) and which of the two it was
    int failed_at() const { std::lock_guard<std::mutex> l(m_); return failed_at_; }
    Status failure() const { std::lock_guard<std::mutex> l(m_); return failure_; }
private:
    int fd_ = -1;
    fav_y4m_stream_header hdr_{};
    size_t frame_bytes_ = 0;
    mutable std::mutex m_;
    std::condition_variable turn_;
    int next_ = 1, failed_at_ = 0;
    bool ended_ = false;
    Status failure_ = END;
};

class Writer {
public:
    ~Writer() { if (fd_ > 1) close(fd_); }
    bool open(const std::string& path)
    {
        fd_ = path == "-" ? 1 : ::open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0666);
        return fd_ >= 0;
    }
    bool header(const fav_y4m_stream_header& h)
    {
        char buf[FAV_Y4M_MAX_HEADER + 1];
        const int n = fav_y4m_format_stream_header_host(&h, buf, sizeof buf);
        return n > 0 && write_full(fd_, buf, (size_t)n);
    }
    bool frame(const uint8_t* planes, size_t n) { return write_full(fd_, "FRAME\n", 6) && write_full(fd_, planes, n); }
private:
    int fd_ = -1;
};

}  // namespace favy
