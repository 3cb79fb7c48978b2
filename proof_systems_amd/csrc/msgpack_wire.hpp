// msgpack_wire.hpp -- the msgpack framing rmp-serde gives a ProverProof and a VerifierIndex, for proof_wire.hpp and the kh_*_msgpack calls (proof_msgpack.cpp).
// The subset those two structures use and nothing else:
//     nil 0xc0 | false 0xc2 | true 0xc3 | positive fixint 0x00-0x7f | uint8/16/32/64 0xcc-0xcf | bin8/16/32 0xc4-0xc6 | fixarray 0x90-0x9f | array16/32 0xdc 0xdd
// Maps, strings, extensions, floats, negative integers and the reserved byte 0xc1 are refused.  Plain host C++ over byte buffers: no device type, no library
// state, so a stand-alone program can walk it under sanitizers (tests/cpp/test_msgpack_wire.cpp).  Every length is checked against the bytes that remain
// before a read and before anything is sized by it (an array of n entries needs n bytes at least); arrays nest 8 deep at most; an error is the byte offset
// with "expected X, found type byte 0x..", never a read past `len`.  The writer always picks the shortest encoding, which is what rmp-serde writes.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>

namespace kh_msgpack {

constexpr int MAX_DEPTH = 8;

struct Reader {
    const uint8_t* p = nullptr;
    size_t len = 0, pos = 0;
    int depth = 0;
    bool failed = false;
    char err[160] = {0};

    Reader(const uint8_t* bytes, size_t n) : p(bytes), len(bytes ? n : 0) {}
    size_t left() const { return len - pos; }

    // every refusal goes through here; the first one stays
    bool refuse(const char* expected) {
        if (failed) return false;
        failed = true;
        if (pos < len) snprintf(err, sizeof(err), "offset %zu: expected %s, found type byte 0x%02x", pos, expected, p[pos]);
        else snprintf(err, sizeof(err), "offset %zu: expected %s, found the end of the %zu bytes", pos, expected, len);
        return false;
    }
    bool refuse_text(size_t at, const char* text) {
        if (failed) return false;
        failed = true;
        snprintf(err, sizeof(err), "offset %zu: %s", at, text);
        return false;
    }
    // big-endian payload of `n` bytes behind the type byte, checked against what is left
    bool be(size_t n, uint64_t* v, const char* expected) {
        if (left() < 1 + n) { pos = len; return refuse(expected); }              // the payload ends short
        uint64_t x = 0;
        for (size_t i = 0; i < n; i++) x = (x << 8) | p[pos + 1 + i];
        *v = x;
        pos += 1 + n;
        return true;
    }
    bool at_nil() const { return !failed && pos < len && p[pos] == 0xc0; }
    bool nil() {
        if (failed || pos >= len || p[pos] != 0xc0) return refuse("nil");
        pos++;
        return true;
    }
    bool boolean(bool* v) {
        if (failed || pos >= len || (p[pos] != 0xc2 && p[pos] != 0xc3)) return refuse("a bool");
        *v = p[pos++] == 0xc3;
        return true;
    }
    bool uint(uint64_t* v) {
        const char* const what = "an unsigned integer";
        if (failed || pos >= len) return refuse(what);
        const uint8_t t = p[pos];
        if (t < 0x80) { *v = t; pos++; return true; }
        if (t >= 0xcc && t <= 0xcf) return be((size_t)1 << (t - 0xcc), v, what);
        return refuse(what);
    }
    // a bin of any length: a view into the buffer
    bool bin(const uint8_t** bytes, size_t* n) {
        const char* const what = "a bin";
        if (failed || pos >= len) return refuse(what);
        const uint8_t t = p[pos];
        if (t < 0xc4 || t > 0xc6) return refuse(what);
        const size_t at = pos;
        uint64_t cnt = 0;
        if (!be((size_t)1 << (t - 0xc4), &cnt, what)) return false;
        if (cnt > left()) { pos = at; return refuse_text(at, "a bin claims more bytes than the buffer has left"); }
        *bytes = p + pos; *n = (size_t)cnt;
        pos += (size_t)cnt;
        return true;
    }
    // a bin of exactly `want` bytes
    bool bin_of(size_t want, const uint8_t** bytes) {
        const size_t at = pos;
        size_t n = 0;
        if (!bin(bytes, &n)) return false;
        if (n != want) {
            failed = true;
            snprintf(err, sizeof(err), "offset %zu: expected a bin of %zu bytes, found one of %zu", at, want, n);
            return false;
        }
        return true;
    }
    // the header of an array; the caller reads its n entries and then calls leave()
    bool enter(size_t* n) {
        const char* const what = "an array";
        if (failed || pos >= len) return refuse(what);
        const uint8_t t = p[pos];
        const size_t at = pos;
        uint64_t cnt = 0;
        if ((t & 0xf0) == 0x90) { cnt = t & 0x0f; pos++; }
        else if (t == 0xdc) { if (!be(2, &cnt, what)) return false; }
        else if (t == 0xdd) { if (!be(4, &cnt, what)) return false; }
        else return refuse(what);
        if (cnt > left()) { pos = at; return refuse_text(at, "an array claims more entries than the buffer has bytes left"); }
        if (depth >= MAX_DEPTH) { pos = at; return refuse_text(at, "arrays nested deeper than 8"); }
        depth++;
        *n = (size_t)cnt;
        return true;
    }
    bool enter_of(size_t want, const char* what) {
        const size_t at = pos;
        size_t n = 0;
        if (!enter(&n)) return false;
        if (n != want) {
            failed = true;
            snprintf(err, sizeof(err), "offset %zu: %s: an array of %zu entries expected, found %zu", at, what, want, n);
            return false;
        }
        return true;
    }
    void leave() { if (!failed && depth > 0) depth--; }
    // any one value of the subset, walked and dropped
    bool skip() {
        if (failed || pos >= len) return refuse("a value");
        const uint8_t t = p[pos];
        if (t == 0xc0) return nil();
        if (t == 0xc2 || t == 0xc3) { bool b; return boolean(&b); }
        if (t < 0x80 || (t >= 0xcc && t <= 0xcf)) { uint64_t v; return uint(&v); }
        if (t >= 0xc4 && t <= 0xc6) { const uint8_t* b; size_t n; return bin(&b, &n); }
        if ((t & 0xf0) == 0x90 || t == 0xdc || t == 0xdd) {
            size_t n = 0;
            if (!enter(&n)) return false;
            for (size_t i = 0; i < n; i++) if (!skip()) return false;
            leave();
            return true;
        }
        return refuse("nil, a bool, an unsigned integer, a bin or an array");
    }
    // after the top-level object: nothing may follow
    bool finish() {
        if (failed) return false;
        if (pos != len) return refuse("the end of the buffer");
        return true;
    }
};

struct Writer {
    std::vector<uint8_t> out;
    void be(uint64_t v, int n) { for (int i = n - 1; i >= 0; i--) out.push_back((uint8_t)(v >> (8 * i))); }
    void nil() { out.push_back(0xc0); }
    void boolean(bool v) { out.push_back(v ? 0xc3 : 0xc2); }
    void uint(uint64_t v) {
        if (v < 0x80) out.push_back((uint8_t)v);
        else if (v <= 0xff) { out.push_back(0xcc); be(v, 1); }
        else if (v <= 0xffff) { out.push_back(0xcd); be(v, 2); }
        else if (v <= 0xffffffffu) { out.push_back(0xce); be(v, 4); }
        else { out.push_back(0xcf); be(v, 8); }
    }
    void bin(const uint8_t* bytes, size_t n) {
        if (n <= 0xff) { out.push_back(0xc4); be(n, 1); }
        else if (n <= 0xffff) { out.push_back(0xc5); be(n, 2); }
        else { out.push_back(0xc6); be(n, 4); }
        out.insert(out.end(), bytes, bytes + n);
    }
    void array(size_t n) {
        if (n <= 15) out.push_back((uint8_t)(0x90 | n));
        else if (n <= 0xffff) { out.push_back(0xdc); be(n, 2); }
        else { out.push_back(0xdd); be(n, 4); }
    }
};

}  // namespace kh_msgpack
