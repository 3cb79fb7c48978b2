// The framing of an SRS file (proof_systems_amd/csrc/srs_file.hpp) on the host, alone: no device, no library.  tests/test_srs_file.py builds this
// with -fsanitize=address,undefined and runs it.  Every buffer handed to the reader is a heap block of EXACTLY the length it is told, so a read past
// that length is a sanitizer report, not luck.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../proof_systems_amd/csrc/srs_file.hpp"

namespace F = kh_srs_file;

static int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } \
    } while (0)

// parse() over an exact-size copy of file[0, len)
static int parse_exact(const std::vector<uint8_t>& file, size_t len, F::View* v, char* err, size_t cap, uint8_t** keep = nullptr) {
    uint8_t* block = (uint8_t*)malloc(len ? len : 1);
    if (len) memcpy(block, file.data(), len);
    const int rc = F::parse(block, len, v, err, cap);
    if (keep && rc == 0) *keep = block; else free(block);
    return rc;
}

int main() {
    char err[192];
    CHECK(F::file_bytes(0) == 41 && F::file_bytes(1) == 76 && F::file_bytes(65536) == 6 + 35 * (size_t)65537);
    CHECK(F::file_bytes(SIZE_MAX) == 0 && F::file_bytes(SIZE_MAX / 35) == 0);
    for (size_t n : {(size_t)0, (size_t)1, (size_t)5, (size_t)300}) {
        std::vector<uint8_t> g(n * F::RECORD), h(F::RECORD);
        for (size_t i = 0; i < g.size(); i++) g[i] = (uint8_t)(i * 131 + 7);
        for (size_t i = 0; i < h.size(); i++) h[i] = (uint8_t)(0xf0 ^ i);
        const size_t len = F::file_bytes(n);
        std::vector<uint8_t> file(len, 0xee);
        // a buffer one byte short is refused and left alone
        CHECK(F::write(g.data(), n, h.data(), file.data(), len - 1, err, sizeof err) == -1 && file[0] == 0xee);
        CHECK(F::write(g.data(), n, h.data(), file.data(), len, err, sizeof err) == 0);
        CHECK(file[0] == 0x92 && file[1] == 0xdd && file[2] == 0 && file[3] == 0 && file[4] == (uint8_t)(n >> 8) && file[5] == (uint8_t)n);
        // the round trip
        F::View v;
        uint8_t* block = nullptr;
        CHECK(parse_exact(file, len, &v, err, sizeof err, &block) == 0 && block);
        if (block) {
            CHECK(v.count == n);
            for (size_t i = 0; i < n; i++) CHECK(memcmp(v.record(i), g.data() + i * F::RECORD, F::RECORD) == 0);
            CHECK(memcmp(v.record(n), h.data(), F::RECORD) == 0);
            free(block);
        }
        // every truncation is refused, with a message, without a read past the end
        for (size_t cut = 0; cut < len; cut++) {
            err[0] = 0;
            CHECK(parse_exact(file, cut, &v, err, sizeof err) == -1 && strstr(err, "offset"));
        }
        // a surplus byte, a count one too large or too small
        std::vector<uint8_t> longer(file); longer.push_back(0);
        CHECK(parse_exact(longer, longer.size(), &v, err, sizeof err) == -1);
        std::vector<uint8_t> more(file); more[5]++;
        CHECK(parse_exact(more, more.size(), &v, err, sizeof err) == -1 && strstr(err, "offset"));
        if (n) {
            std::vector<uint8_t> fewer(file); fewer[5]--;
            CHECK(parse_exact(fewer, fewer.size(), &v, err, sizeof err) == -1);
        }
        // every marker byte
        for (size_t at : {(size_t)0, (size_t)1}) {
            std::vector<uint8_t> bad(file); bad[at] ^= 1;
            CHECK(parse_exact(bad, bad.size(), &v, err, sizeof err) == -1 && strstr(err, "offset"));
        }
        for (size_t i = 0; i <= n; i++)
            for (size_t k = 0; k < 2; k++) {
                std::vector<uint8_t> bad(file); bad[F::HEADER + F::ITEM * i + k] ^= 0x10;
                err[0] = 0;
                CHECK(parse_exact(bad, bad.size(), &v, err, sizeof err) == -1 && strstr(err, "offset"));
            }
    }
    // a count whose size does not fit is refused on the header alone
    {
        std::vector<uint8_t> head = {0x92, 0xdd, 0xff, 0xff, 0xff, 0xff};
        F::View v;
        CHECK(parse_exact(head, head.size(), &v, err, sizeof err) == -1);
    }
    F::View v;
    CHECK(F::parse(nullptr, 0, &v, err, sizeof err) == -1);
    if (failures) { printf("%d checks failed\n", failures); return 1; }
    printf("srs_file OK\n");
    return 0;
}
