// textfile_check.cpp - fhx::TextFile (fithic_amd/csrc/fhx_textfile.hpp), the HIP-free reader under the device text paths, run on
// its own under AddressSanitizer + UndefinedBehaviorSanitizer.
//
// Linked against fhx_io.cpp and fhx_gunzip.cpp compiled with
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -pthread
// (tests/test_sanitizers.py builds and runs it).  Sizes round the 4 MiB pread slice, ranges that split inside a slice, the
// last-newline offset, what open() refuses, and a gzip file with gzip allowed and not.
//
//     textfile_check <scratch dir>
#include <fcntl.h>
#include <unistd.h>
#include <zlib.h>

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "fhx_textfile.hpp"

static long failures = 0;
#define EXPECT(cond, what)                                                                   \
    do {                                                                                     \
        if (!(cond)) {                                                                       \
            std::fprintf(stderr, "CHECK FAILED line %d: %s (%s)\n", __LINE__, #cond, what); \
            ++failures;                                                                      \
        }                                                                                    \
    } while (0)

static void put(const std::string& path, const std::string& bytes) {
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f || std::fwrite(bytes.data(), 1, bytes.size(), f) != bytes.size()) std::abort();
    std::fclose(f);
}

// bytes [off, off + len) of the file with plain read()
static std::string plain_read(const std::string& path, int64_t off, int64_t len) {
    std::string out((size_t)len, '\0');
    const int fd = ::open(path.c_str(), O_RDONLY);
    if (fd < 0 || ::lseek(fd, (off_t)off, SEEK_SET) != (off_t)off) std::abort();
    for (int64_t at = 0; at < len;) {
        const ssize_t got = ::read(fd, &out[(size_t)at], (size_t)(len - at));
        if (got <= 0) std::abort();
        at += got;
    }
    ::close(fd);
    return out;
}

// no newline anywhere: `seed` only varies the bytes
static std::string pattern(size_t n, unsigned seed) {
    std::string s(n, '\0');
    unsigned x = seed * 2654435761u + 1;
    for (size_t i = 0; i < n; ++i) {
        x = x * 1664525u + 1013904223u;
        s[i] = (char)('a' + (x >> 24) % 26);
    }
    return s;
}

// the range through TextFile::read, in a buffer of exactly len bytes (an overrun is the sanitizer's to report)
static std::string range(const fhx::TextFile& f, int64_t off, int64_t len, int64_t* last_newline) {
    std::vector<char> buf((size_t)len);
    EXPECT(f.read(off, len, buf.data(), last_newline) == 0, "read");
    return std::string(buf.data(), buf.size());
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string dir = argv[1];
    const std::string path = dir + "/text";
    std::string err;
    const int64_t slice = (int64_t)4 << 20;
    int64_t nl = 0;

    // whole files round the slice edge
    const int64_t sizes[] = {0, 1, slice - 1, slice, slice + 1};
    for (int64_t n : sizes) {
        std::string text = pattern((size_t)n, (unsigned)n);
        if (n > 0) text[(size_t)n / 2] = '\n';
        put(path, text);
        fhx::TextFile f;
        EXPECT(f.open(path.c_str(), true, &err) == FHX_OK && err.empty(), "open");
        EXPECT(f.size() == n, "size");
        EXPECT(range(f, 0, n, &nl) == text, "the whole file");
        EXPECT(nl == (n > 0 ? n / 2 : -1), "last newline of the whole file");
    }

    // about 9 MiB as two ranges that split inside the second slice
    {
        const int64_t n = 9 * ((int64_t)1 << 20) + 12345, cut = slice + 777777;
        const std::string text = pattern((size_t)n, 9);
        put(path, text);
        fhx::TextFile f;
        EXPECT(f.open(path.c_str(), false, &err) == FHX_OK, "open");
        EXPECT(range(f, 0, cut, &nl) == plain_read(path, 0, cut) && nl == -1, "first range");
        EXPECT(range(f, cut, n - cut, &nl) == plain_read(path, cut, n - cut) && nl == -1, "second range");
    }

    // the last newline of a range: none, at its first byte, at its last byte, and the last of several
    {
        std::string text = pattern(3000, 3);
        text[1000] = text[1999] = '\n';
        put(path, text);
        fhx::TextFile f;
        EXPECT(f.open(path.c_str(), true, &err) == FHX_OK, "open");
        range(f, 0, 1000, &nl);
        EXPECT(nl == -1, "no newline");
        range(f, 1000, 999, &nl);
        EXPECT(nl == 0, "newline at byte 0");
        range(f, 1001, 999, &nl);
        EXPECT(nl == 998, "newline at the last byte");
        range(f, 0, 3000, &nl);
        EXPECT(nl == 1999, "the last of two");
        range(f, 500, 0, &nl);
        EXPECT(nl == -1, "an empty range");
    }

    // what open() refuses
    {
        fhx::TextFile d;
        err.clear();
        EXPECT(d.open(dir.c_str(), true, &err) == FHX_ERR_ARG && err == dir + ": not a regular file", err.c_str());
        fhx::TextFile m;
        const std::string missing = dir + "/no such file";
        err.clear();
        EXPECT(m.open(missing.c_str(), true, &err) == FHX_ERR_ARG && err.rfind(missing + ": ", 0) == 0 && err.size() > missing.size() + 2, err.c_str());
    }

    // a gzip file: its text with gzip allowed, the bytes it holds without
    {
        std::string text;
        for (int i = 0; i < 5000; ++i) text += "chr1\t" + std::to_string(5000 * i) + "\tchr1\t" + std::to_string(5000 * i + 40000) + "\t7\n";
        const std::string gz = dir + "/text.gz";
        gzFile g = gzopen(gz.c_str(), "wb");
        if (!g || gzwrite(g, text.data(), (unsigned)text.size()) != (int)text.size() || gzclose(g) != Z_OK) std::abort();
        fhx::TextFile f;
        err.clear();
        EXPECT(f.open(gz.c_str(), true, &err) == FHX_OK && err.empty(), err.c_str());
        EXPECT(f.size() == (int64_t)text.size(), "inflated size");
        EXPECT(range(f, 0, f.size(), &nl) == text && nl == f.size() - 1, "inflated text");
        EXPECT(range(f, 100, 1000, &nl) == text.substr(100, 1000), "a range of the inflated text");
        f.release();
        fhx::TextFile raw;
        EXPECT(raw.open(gz.c_str(), false, &err) == FHX_OK, "open raw");
        const std::string bytes = plain_read(gz, 0, raw.size());
        EXPECT(raw.size() < (int64_t)text.size() && (unsigned char)bytes[0] == 0x1f && (unsigned char)bytes[1] == 0x8b, "the gzip container");
        EXPECT(range(raw, 0, raw.size(), &nl) == bytes, "raw bytes");
        // a file that only starts like gzip is an error where gzip is allowed, and plain bytes where it is not
        const std::string fake = "\x1f\x8b not deflate at all\n";
        put(path, fake);
        fhx::TextFile bad, plain;
        err.clear();
        EXPECT(bad.open(path.c_str(), true, &err) != FHX_OK && !err.empty(), "a broken gzip file says why");
        EXPECT(plain.open(path.c_str(), false, &err) == FHX_OK && plain.size() == (int64_t)fake.size(), "the same bytes read raw");
    }

    std::printf("textfile_check: %ld check failures\n", failures);
    return failures ? 1 : 0;
}
