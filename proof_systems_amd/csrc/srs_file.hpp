// srs_file.hpp -- the framing of an SRS file, for kh_srs_write_file and kh_srs_create_from_file (srs.cpp):
//     0x92 | 0xdd count (big-endian u32) | count x (0xc4 0x21 record) | 0xc4 0x21 record of h          a record: 33 bytes (include/kimchi_hip.h)
// Plain host C++ over byte buffers: no device type, no library state, so a stand-alone program can walk it under sanitizers
// (tests/cpp/test_srs_file.cpp).  Every length is checked before a read; an error is a message with the byte offset, never a read past `len`.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

namespace kh_srs_file {

constexpr size_t RECORD = 33, ITEM = 2 + RECORD, HEADER = 6;
constexpr uint8_t ARRAY2 = 0x92, ARRAY32 = 0xdd, BIN8 = 0xc4;

// 6 + 35 (n + 1), or 0 when that does not fit a size_t
inline size_t file_bytes(size_t n) {
    if (n >= (SIZE_MAX - HEADER) / ITEM) return 0;
    return HEADER + ITEM * (n + 1);
}

struct View {
    size_t count = 0;                  // the points of g; h is item `count`
    const uint8_t* items = nullptr;    // count + 1 items of ITEM bytes
    const uint8_t* record(size_t i) const { return items + ITEM * i + 2; }      // i <= count
};

// 0, or -1 with `err` filled in
inline int parse(const uint8_t* file, size_t len, View* out, char* err, size_t err_cap) {
    if (!file || !out) { snprintf(err, err_cap, "SRS file: null argument"); return -1; }
    if (len < HEADER) { snprintf(err, err_cap, "SRS file: %zu bytes end inside the header, at offset %zu", len, len); return -1; }
    if (file[0] != ARRAY2) { snprintf(err, err_cap, "SRS file: byte 0x%02x at offset 0 is not the marker 0x92", file[0]); return -1; }
    if (file[1] != ARRAY32) { snprintf(err, err_cap, "SRS file: byte 0x%02x at offset 1 is not the marker 0xdd", file[1]); return -1; }
    const size_t count = ((size_t)file[2] << 24) | ((size_t)file[3] << 16) | ((size_t)file[4] << 8) | (size_t)file[5];
    const size_t want = file_bytes(count);
    if (want == 0 || want != len) {
        const size_t at = want && want < len ? want : len;          // where the file ends short, or where the surplus begins
        snprintf(err, err_cap, "SRS file: a count of %zu points needs %zu bytes, the buffer has %zu (offset %zu)", count, want, len, at);
        return -1;
    }
    for (size_t i = 0; i <= count; i++) {
        const size_t off = HEADER + ITEM * i;                       // off + ITEM <= want == len
        if (file[off] != BIN8 || file[off + 1] != RECORD) {
            snprintf(err, err_cap, "SRS file: bytes 0x%02x 0x%02x at offset %zu are not the marker 0xc4 0x21 of item %zu", file[off], file[off + 1], off, i);
            return -1;
        }
    }
    out->count = count;
    out->items = file + HEADER;
    return 0;
}

// n records of g (33 bytes apart) and the record of h into out[0, file_bytes(n)); 0, or -1 with `err` filled in
inline int write(const uint8_t* g_records, size_t n, const uint8_t* h_record, uint8_t* out, size_t cap, char* err, size_t err_cap) {
    if ((!g_records && n) || !h_record || !out) { snprintf(err, err_cap, "SRS file: null argument"); return -1; }
    const size_t want = file_bytes(n);
    if (n > 0xffffffffu || want == 0) { snprintf(err, err_cap, "SRS file: %zu points do not fit the u32 count", n); return -1; }
    if (cap < want) { snprintf(err, err_cap, "SRS file: %zu points need %zu bytes, the buffer has %zu", n, want, cap); return -1; }
    out[0] = ARRAY2; out[1] = ARRAY32;
    out[2] = (uint8_t)(n >> 24); out[3] = (uint8_t)(n >> 16); out[4] = (uint8_t)(n >> 8); out[5] = (uint8_t)n;
    for (size_t i = 0; i <= n; i++) {
        uint8_t* o = out + HEADER + ITEM * i;
        o[0] = BIN8; o[1] = (uint8_t)RECORD;
        memcpy(o + 2, i < n ? g_records + RECORD * i : h_record, RECORD);
    }
    return 0;
}

}  // namespace kh_srs_file
