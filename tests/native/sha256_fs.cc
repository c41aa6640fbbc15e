// The message layout and the reduction of bls_amd/csrc/sha256_fs.h on the host (tests/test_blob_wire_cpu.py compiles this with the address
// and undefined-behaviour sanitizers and runs it directly).  Reads commands on stdin and answers each with lines of hex digits:
//   hash l a BLOB COMM     l <= 16; a: the offset (0 .. 15) of both buffers from a 16-byte aligned address; BLOB: the 2^l * 32 bytes of the
//                          blob and COMM: the 48 bytes of the commitment, as hex digits.  Two lines: the digest, z.  The buffers hold exactly
//                          the bytes the layout may name (an allocation each that ends with their last byte: the sanitizer sees a byte beyond them).
//   layout l               for every block and word one line `src v` (sha256_fs.h: Word), then one line: the number of blocks
// The whole-message hash is serial over a compression function of this file's own.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../bls_amd/csrc/sha256_fs.h"

using namespace blsmi_fs;

static const uint32_t K[64] = {
    0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3,
    0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da,
    0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13,
    0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070,
    0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208,
    0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};

static uint32_t rotr(uint32_t x, int n) { return x >> n | x << (32 - n); }
static void compress(uint32_t h[8], const uint32_t win[16]) {
    uint32_t w[64];
    for (int i = 0; i < 16; i++) w[i] = win[i];
    for (int i = 16; i < 64; i++) {
        const uint32_t s0 = rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3), s1 = rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10);
        w[i] = w[i - 16] + s0 + w[i - 7] + s1;
    }
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
    for (int i = 0; i < 64; i++) {
        const uint32_t t1 = hh + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) + K[i] + w[i];
        const uint32_t t2 = (rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
        hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
    }
    h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
}
static uint32_t be_word(const uint8_t* p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }

// hex digits into exactly n bytes at out
static bool unhex(const std::string& s, uint8_t* out, size_t n) {
    if (s.size() != 2 * n) return false;
    for (size_t i = 0; i < n; i++) {
        unsigned v;
        if (sscanf(s.c_str() + 2 * i, "%2x", &v) != 1) return false;
        out[i] = (uint8_t)v;
    }
    return true;
}
static bool token(std::string& out) {
    out.clear();
    int ch;
    while ((ch = getchar()) != EOF && (ch == ' ' || ch == '\n')) {}
    if (ch == EOF) return false;
    do out.push_back((char)ch); while ((ch = getchar()) != EOF && ch != ' ' && ch != '\n');
    return true;
}
// a buffer of n bytes whose first byte lies `off` bytes behind a 16-byte aligned address and whose last byte is the allocation's last
struct Placed {
    uint8_t* base; uint8_t* p;
    Placed(size_t n, unsigned off) : base((uint8_t*)malloc(n + off)), p(base + off) { if (!base || ((uintptr_t)base & 15)) abort(); }
    ~Placed() { free(base); }
    Placed(const Placed&) = delete;
    Placed& operator=(const Placed&) = delete;
};

int main() {
    std::string cmd, a, b;
    while (token(cmd)) {
        if (cmd == "hash") {
            unsigned l, off;
            if (!token(a) || !token(b)) return 2;
            l = (unsigned)atoi(a.c_str()); off = (unsigned)atoi(b.c_str());
            if (l > MAX_LOG2N || off > 15) return 2;
            const size_t nbytes = (size_t)32 << l;
            Placed blob(nbytes, off), comm(48, off);
            if (!token(a) || !unhex(a, blob.p, nbytes) || !token(b) || !unhex(b, comm.p, 48)) return 2;
            uint32_t h[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
            for (uint32_t i = 0; i < blocks(l); i++) {
                uint32_t w[16];
                for (uint32_t k = 0; k < 16; k++) {
                    const Word s = word(l, i, k);
                    if (s.src == FS_CONST) w[k] = s.v;
                    else {
                        if (s.v + 4 > (s.src == FS_BLOB ? nbytes : 48)) return 3;
                        w[k] = be_word((s.src == FS_BLOB ? blob.p : comm.p) + s.v);
                    }
                    if (whole_in_blob(l, i) && (s.src != FS_BLOB || s.v != 64 * i - 32 + 4 * k)) return 3;   // the contiguous form names the same bytes
                }
                compress(h, w);
            }
            for (int k = 0; k < 8; k++) printf("%08x", h[k]);
            printf("\n");
            uint32_t v[8];
            digest_to_scalar(h, v);
            for (int k = 7; k >= 0; k--) printf("%08x", v[k]);
            printf("\n");
        } else if (cmd == "layout") {
            if (!token(a)) return 2;
            const unsigned l = (unsigned)atoi(a.c_str());
            if (l > MAX_LOG2N) return 2;
            for (uint32_t i = 0; i < blocks(l); i++)
                for (uint32_t k = 0; k < 16; k++) { const Word s = word(l, i, k); printf("%u %x\n", s.src, s.v); }
            printf("%u\n", blocks(l));
        } else return 2;
    }
    return 0;
}
