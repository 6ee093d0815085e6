// fhx_textfile.hpp - a text file as the device text paths read it (no HIP here: host compilers take this header as it is).
//
// The source is a regular file read with pread, or, when the caller allows it and the file starts with the gzip magic, its
// inflated bytes (fhx_host_inflate).  read() fills a caller's buffer - a pinned one in fhx_textupload.hpp - with a range of it.
#pragma once
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <cstdint>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../include/fithic_mi355x.h"
#include "fhx_cpus.hpp"

namespace fhx {

class TextFile {
  public:
    TextFile() = default;
    TextFile(const TextFile&) = delete;
    TextFile& operator=(const TextFile&) = delete;
    ~TextFile() { close_fd(); }

    // FHX_OK, or the code to return with *err set.  allow_gzip = false reads a gzip file as the bytes it holds.
    int open(const char* path, bool allow_gzip, std::string* err) {
        fd_ = ::open(path, O_RDONLY | O_CLOEXEC);
        if (fd_ < 0) return fail(err, FHX_ERR_ARG, std::string(path) + ": " + std::strerror(errno));
        struct stat sb;
        if (::fstat(fd_, &sb) != 0 || !S_ISREG(sb.st_mode)) return fail(err, FHX_ERR_ARG, std::string(path) + ": not a regular file");
        size_ = (int64_t)sb.st_size;
        unsigned char magic[2] = {0, 0};
        if (allow_gzip && size_ >= 2 && ::pread(fd_, magic, 2, 0) == 2 && magic[0] == 0x1f && magic[1] == 0x8b) {
            fhx_text* x = nullptr;
            int rc = fhx_host_inflate(path, 0, &x);
            if (rc != FHX_OK) {
                const std::string msg = x ? fhx_text_error(x) : "fhx_host_inflate";
                fhx_text_free(x);
                return fail(err, rc, msg);
            }
            inflated_.resize((size_t)fhx_text_bytes(x));
            rc = fhx_text_copy(x, inflated_.data(), (int64_t)inflated_.size());
            fhx_text_free(x);
            if (rc != FHX_OK) return fail(err, rc, "fhx_text_copy");
            close_fd();
            size_ = (int64_t)inflated_.size();
        }
        return FHX_OK;
    }

    int64_t size() const { return size_; }                                    // of the text: inflated, for a gzip file

    // Bytes [off, off + len) of the text -> dst: a memcpy of inflated bytes, or up to min(usable_cpus(), 8) threads doing pread
    // in 4 MB slices.  0, or the errno of the read that failed (EIO when the file shrank under us).  *last_newline = the offset
    // within the range of its last newline, -1 without one.
    int read(int64_t off, int64_t len, char* dst, int64_t* last_newline) const {
        *last_newline = -1;
        if (fd_ < 0) {
            if (len > 0) std::memcpy(dst, inflated_.data() + off, (size_t)len);
        } else {
            const int64_t slice = (int64_t)4 << 20;
            const int64_t n_slices = (len + slice - 1) / slice;
            std::atomic<int64_t> next{0};
            std::atomic<int> io_errno{0};
            auto work = [&]() {
                for (;;) {
                    const int64_t s = next.fetch_add(1);
                    if (s >= n_slices) return;
                    int64_t at = s * slice;
                    const int64_t stop = std::min(len, at + slice);
                    while (at < stop) {
                        const ssize_t got = ::pread(fd_, dst + at, (size_t)(stop - at), (off_t)(off + at));
                        if (got < 0 && errno == EINTR) continue;
                        if (got <= 0) {                                       // an error, or the file shrank under us
                            io_errno = got < 0 ? errno : EIO;
                            return;
                        }
                        at += got;
                    }
                }
            };
            const int nt = (int)std::max<int64_t>(1, std::min<int64_t>(std::min(usable_cpus(), 8), n_slices));
            std::vector<std::thread> pool;
            for (int k = 1; k < nt; ++k) pool.emplace_back(work);
            work();
            for (auto& th : pool) th.join();
            if (io_errno) return io_errno;
        }
        if (len > 0)
            if (const void* nl = ::memrchr(dst, '\n', (size_t)len)) *last_newline = (const char*)nl - dst;
        return 0;
    }

    // the inflated bytes are not needed once the last range has been read
    void release() { std::vector<char>().swap(inflated_); }

  private:
    static int fail(std::string* err, int code, const std::string& msg) {
        *err = msg;
        return code;
    }
    void close_fd() {
        if (fd_ >= 0) ::close(fd_);
        fd_ = -1;
    }
    int fd_ = -1;
    std::vector<char> inflated_;
    int64_t size_ = 0;
};

}  // namespace fhx
