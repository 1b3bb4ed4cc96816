// Stand-alone check of csrc/lnb_wpack.h (the lossless 13-bit planar copy of a bf16 weight matrix) on the host, built under the address and
// undefined-behaviour sanitizers by tests/test_wpack_cpu.py:
//   1. every one of the 65536 bf16 patterns, in a matrix whose window admits it (at the window's lower end and at its upper end), survives pack -> unpack;
//   2. a matrix with a subnormal, an exponent of 1, an Inf, a NaN or a weight one step outside the window is refused with its reason;
//   3. the decode the kernel runs -- spread, add, sign, byte permute, four weights at a time -- gives the scalar definition's bits.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../llama-nuts-and-bolts_amd/csrc/lnb_wpack.h"

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails++ < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static int window_of(const std::vector<uint16_t>& m, uint32_t* base) {
    WpackStats s; wpack_stats_init(&s);
    for (uint16_t w : m) wpack_stats_add(&s, w);
    return wpack_window(&s, base);
}
// the kernel's order: pair pi, chain c, half h -> quad g = 4 pi + 2 c + h, code dword u = 2 pi + c
static void decode_swar(const uint32_t* low8, const uint32_t* code4, uint32_t sign1, uint32_t base, uint16_t* out) {
    const uint32_t base4 = base * 0x01010101u;
    for (int pi = 0; pi < 2; pi++)
        for (int c = 0; c < 2; c++)
            for (int h = 0; h < 2; h++) {
                const int g = 4 * pi + 2 * c + h;
                const uint32_t hi = wpack_hi4(wpack_spread(code4[2 * pi + c], h), sign1, g, base4), lo = low8[g];
                const uint32_t f[4] = {wpack_wide<0>(hi, lo), wpack_wide<1>(hi, lo), wpack_wide<2>(hi, lo), wpack_wide<3>(hi, lo)};
                for (int j = 0; j < 4; j++) {
                    CHECK((f[j] & 0xFFFFu) == 0, "low half of a widened weight not zero");
                    out[4 * g + j] = (uint16_t)(f[j] >> 16);
                }
            }
}
// pack the matrix (a whole number of groups) with its own window and compare both decodes with the input
static void roundtrip(const std::vector<uint16_t>& m, const char* what) {
    uint32_t base = 0;
    const int why = window_of(m, &base);
    CHECK(why == WPACK_OK, "%s: refused (%d)", what, why);
    if (why != WPACK_OK) return;
    for (size_t o = 0; o + WPACK_GROUP <= m.size(); o += WPACK_GROUP) {
        uint32_t low8[8], code4[4], sg;
        uint16_t a[WPACK_GROUP], b[WPACK_GROUP];
        wpack_pack_group(&m[o], base, low8, code4, &sg);
        wpack_unpack_group(low8, code4, sg, base, a);
        decode_swar(low8, code4, sg, base, b);
        for (int i = 0; i < WPACK_GROUP; i++) {
            CHECK(a[i] == m[o + i], "%s: scalar unpack %04x -> %04x (base %u)", what, m[o + i], a[i], base);
            CHECK(b[i] == m[o + i], "%s: kernel decode %04x -> %04x (base %u)", what, m[o + i], b[i], base);
        }
    }
}
static uint16_t bf(uint32_t sign, uint32_t exp, uint32_t man) { return (uint16_t)((sign << 15) | (exp << 7) | man); }
static uint32_t rnd_state = 12345;
static uint32_t rnd() { rnd_state = rnd_state * 1664525u + 1013904223u; return rnd_state >> 8; }

int main() {
    // 1. every pattern
    long packed = 0, skipped = 0;
    for (uint32_t p = 0; p < 65536; p++) {
        const uint32_t e = (p >> 7) & 0xFF;
        if (e == 0xFF || (e < 2 && (p & 0x7FFF))) { skipped++; continue; }           // not packable in any window: case 2
        const int e2 = (int)(e >> 1);
        for (int end = 0; end < 2; end++) {
            std::vector<uint16_t> m(WPACK_GROUP, 0);
            for (int i = 0; i < WPACK_GROUP; i++) m[i] = (i & 1) ? 0x8000 : 0x0000;   // both zeros around it
            m[rnd() % WPACK_GROUP] = (uint16_t)p;
            if (e >= 2) {
                const int other = end == 0 ? e2 + 14 : e2 - 14;                       // p at the lower / upper end of a full window
                if (other >= 1 && other <= 127) {
                    int at = (int)(rnd() % WPACK_GROUP);
                    while (m[at] == (uint16_t)p) at = (at + 1) % WPACK_GROUP;
                    uint32_t oe = (uint32_t)other * 2 + (end == 0 ? 1 : 0);
                    if (oe > 254) oe = 254;
                    m[at] = bf(rnd() & 1, oe, rnd() & 0x7F);
                }
            }
            roundtrip(m, "every pattern");
        }
        packed++;
    }
    CHECK(packed == 65536 - 2 * (128 + 127 + 128), "patterns packed: %ld (skipped %ld)", packed, skipped);
    // 2. refusals
    {
        struct { uint16_t w; int why; const char* what; } bad[] = {
            {0x0001, WPACK_SUBNORMAL, "smallest subnormal"}, {0x807F, WPACK_SUBNORMAL, "largest negative subnormal"},
            {0x0080, WPACK_SUBNORMAL, "exponent 1"}, {0x80FF, WPACK_SUBNORMAL, "exponent 1, negative, full mantissa"},
            {0x7F80, WPACK_INFNAN, "+Inf"}, {0xFF80, WPACK_INFNAN, "-Inf"}, {0x7FC1, WPACK_INFNAN, "NaN"}};
        for (auto& b : bad) {
            std::vector<uint16_t> m(2 * WPACK_GROUP);
            for (auto& w : m) w = bf(rnd() & 1, 110 + rnd() % 16, rnd() & 0x7F);
            m[rnd() % m.size()] = b.w;
            uint32_t base;
            CHECK(window_of(m, &base) == b.why, "%s: not refused as %d", b.what, b.why);
        }
        for (int lo = 1; lo + 15 <= 127; lo += 7) {
            std::vector<uint16_t> m(WPACK_GROUP, 0);
            m[3] = bf(0, 2 * lo, 0); m[9] = bf(1, 2 * (lo + 14) + 1, 0x7F);
            uint32_t base;
            CHECK(window_of(m, &base) == WPACK_OK && base == (uint32_t)lo - 1, "full window at %d refused", lo);
            roundtrip(m, "full window");
            m[20] = bf(0, 2 * (lo + 15), 0);                                          // one binade pair above the window
            CHECK(window_of(m, &base) == WPACK_WINDOW, "weight above the window at %d not refused", lo);
            m[20] = 0; m[9] = bf(1, 2 * (lo + 15) + 1, 1);
            CHECK(window_of(m, &base) == WPACK_WINDOW, "window of 16 codes at %d not refused", lo);
        }
        std::vector<uint16_t> z(WPACK_GROUP, 0x8000);
        uint32_t base = 99;
        CHECK(window_of(z, &base) == WPACK_OK && base == 0, "all-zero matrix");
        roundtrip(z, "all -0");
    }
    // 3. the kernel's decode against the scalar definition
    for (int trial = 0; trial < 20000; trial++) {
        const int kind = trial % 6, lo = 1 + (int)(rnd() % 113);                      // window [lo, lo + 14]
        std::vector<uint16_t> m(WPACK_GROUP);
        for (int i = 0; i < WPACK_GROUP; i++) {
            uint32_t e2 = lo + rnd() % 15, s = rnd() & 1, zero = (rnd() % 8) == 0;
            if (kind == 1) zero = 1;                                                  // only code 0
            if (kind == 2) { e2 = lo + 14; zero = 0; }                                // only code 15
            if (kind == 3) s = 1;                                                     // all signs set
            if (kind == 4) s = i & 1;                                                 // alternating signs
            if (kind == 5) s = (i >> 2) & 1;                                          // alternating by quad
            const uint32_t ex = 2 * e2 + (rnd() & 1);                                  // (exponent 255 is Inf / NaN: the top binade pair has one member)
            m[i] = zero ? (uint16_t)(s << 15) : bf(s, ex > 254 ? 254 : ex, rnd() & 0x7F);
        }
        if (kind == 2) m[0] = bf(0, 2 * lo, 0);                                       // ... with the window's lower end pinned so that the rest is code 15
        roundtrip(m, "random groups");
    }
    // stream geometry
    CHECK(wpack_stage_bytes(448) == 23296 && wpack_stages(4096, 448, 56) == 32 && wpack_stages(256, 448, 56) == 2 && wpack_stages(264, 448, 56) == 3, "stage geometry");
    CHECK(wpack_bytes(256, 4096, 448, 56) * 16 == (size_t)256 * 2 * 56 * 4096 * 2 * 13, "the 8B gate|up copy is 13/16 of the matrix");
    if (fails) { printf("wpack_test: %d failures\n", fails); return 1; }
    printf("wpack_test: ok\n");
    return 0;
}
