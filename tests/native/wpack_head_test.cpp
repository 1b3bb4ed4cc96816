// Stand-alone check of the LM head's stream in csrc/lnb_wpack.h on the host, built under the address and undefined-behaviour sanitizers by
// tests/test_wpack_head_cpu.py.  A matrix goes from the resident [N/64][K/8][1][64][8] layout through the head addressing (wpack_head_src_unit,
// wpack_head_stage_off, wpack_plane_off: what the pack kernel runs) into a copy of exactly wpack_head_bytes, and comes back the way the kernel consumes it
// (block, stage, lane -> two (chunk, row) pairs x two chains):
//   1. every weight comes back bit-identical, each exactly once; rows at or beyond N and chunks at or beyond K / 8 come back as +0;
//   2. stage, block and byte counts, including that the 8B head's copy is 13/16 of its matrix.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../llama-nuts-and-bolts_amd/csrc/lnb_wpack.h"

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails++ < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 32); }
// a packable weight: +-0 now and then, else an exponent in a 30-binade window, any sign and mantissa
static uint16_t weight() {
    const uint32_t r = rnd();
    if (r % 11 == 0) return (r & 1) ? 0x8000 : 0x0000;
    const uint32_t e = 100 + (r >> 8) % 30;
    return (uint16_t)(((r >> 3) & 1) << 15 | e << 7 | ((r >> 16) & 0x7F));
}

static void roundtrip(int N, int K) {
    const int kc8 = K / 8, nres = (N + 63) / 64, nb = wpack_head_blocks(N), nst = wpack_head_stages(K), lanes = WPACK_HEAD_LANES;
    std::vector<uint16_t> W((size_t)N * K), res((size_t)nres * kc8 * 64 * 8, 0);
    for (auto& w : W) w = weight();
    for (int n = 0; n < N; n++)
        for (int k = 0; k < K; k++) res[((((size_t)(n / 64) * kc8 + k / 8) * 64) + n % 64) * 8 + k % 8] = W[(size_t)n * K + k];
    WpackStats s; wpack_stats_init(&s);
    for (uint16_t w : res) wpack_stats_add(&s, w);
    uint32_t base = 0;
    CHECK(wpack_window(&s, &base) == WPACK_OK, "N %d K %d: refused", N, K);
    // ---- counts
    CHECK(nb == (N + 127) / 128 && nst == (K + 127) / 128, "N %d K %d: %d blocks, %d stages", N, K, nb, nst);
    CHECK(wpack_stage_bytes(lanes) == 512 * 52, "stage bytes %zu", wpack_stage_bytes(lanes));
    CHECK(wpack_head_bytes(N, K) == (size_t)nb * nst * 512 * 52, "N %d K %d: %zu bytes", N, K, wpack_head_bytes(N, K));
    CHECK(wpack_head_stage_off(K, nb - 1, nst - 1) + wpack_stage_bytes(lanes) == wpack_head_bytes(N, K), "the last stage does not end the copy");
    // ---- pack: what wpack_pack_head_kernel does per (block, stage, lane); the copy is allocated to the byte (the sanitizer sees an overrun)
    std::vector<unsigned char> copy(wpack_head_bytes(N, K), 0xA5);
    for (int b = 0; b < nb; b++)
        for (int st = 0; st < nst; st++)
            for (int L = 0; L < lanes; L++) {
                uint16_t g[WPACK_GROUP];
                for (int u = 0; u < 4; u++) {
                    const long long su = wpack_head_src_unit(N, K, b, st, L, u);
                    CHECK(su >= -1 && su < (long long)nres * kc8 * 64, "source unit %lld out of the resident layout", su);
                    if (su >= 0) memcpy(g + 8 * u, &res[(size_t)su * 8], 16); else memset(g + 8 * u, 0, 16);
                }
                uint32_t low8[8], code4[4], sg;
                wpack_pack_group(g, base, low8, code4, &sg);
                unsigned char* o = copy.data() + wpack_head_stage_off(K, b, st);
                memcpy(o + wpack_plane_off(lanes, 0, L), low8, 16); memcpy(o + wpack_plane_off(lanes, 1, L), low8 + 4, 16);
                memcpy(o + wpack_plane_off(lanes, 2, L), code4, 16); memcpy(o + wpack_plane_off(lanes, 3, L), &sg, 4);
            }
    // ---- unpack as the kernel consumes it: lane L's pair pi is (chunk, row) = (pq / 64, pq % 64), pq = pi * lanes + L; unit 2 pi + c is chain c = row 128 b + 64 c + r
    std::vector<unsigned char> seen((size_t)N * K, 0);
    for (int b = 0; b < nb; b++)
        for (int st = 0; st < nst; st++)
            for (int L = 0; L < lanes; L++) {
                uint32_t low8[8], code4[4], sg; uint16_t g[WPACK_GROUP];
                const unsigned char* o = copy.data() + wpack_head_stage_off(K, b, st);
                memcpy(low8, o + wpack_plane_off(lanes, 0, L), 16); memcpy(low8 + 4, o + wpack_plane_off(lanes, 1, L), 16);
                memcpy(code4, o + wpack_plane_off(lanes, 2, L), 16); memcpy(&sg, o + wpack_plane_off(lanes, 3, L), 4);
                wpack_unpack_group(low8, code4, sg, base, g);
                for (int pi = 0; pi < 2; pi++)
                    for (int c = 0; c < 2; c++) {
                        const int pq = pi * lanes + L, kc = st * 16 + pq / 64, r = pq % 64, n = 128 * b + 64 * c + r;
                        for (int i = 0; i < 8; i++) {
                            const uint16_t got = g[8 * (2 * pi + c) + i];
                            if (n < N && kc < kc8) {
                                const size_t at = (size_t)n * K + (size_t)kc * 8 + i;
                                CHECK(got == W[at], "N %d K %d: row %d k %d: %04x -> %04x", N, K, n, kc * 8 + i, W[at], got);
                                seen[at]++;
                            } else CHECK(got == 0, "N %d K %d: padding at row %d chunk %d is %04x", N, K, n, kc, got);
                        }
                    }
            }
    size_t once = 0;
    for (unsigned char v : seen) once += v == 1;
    CHECK(once == seen.size(), "N %d K %d: %zu of %zu weights streamed exactly once", N, K, once, seen.size());
}

int main() {
    const int Ns[] = {64, 65, 128, 130, 641}, Ks[] = {128, 264, 896};
    for (int N : Ns) for (int K : Ks) roundtrip(N, K);
    // the 8B head: 128256 = 1002 x 128 rows, 4096 = 32 x 128 steps -- no padding, so the copy is 13/16 of the matrix to the byte
    CHECK(wpack_head_blocks(128256) == 1002 && wpack_head_stages(4096) == 32, "8B head: %d blocks, %d stages", wpack_head_blocks(128256), wpack_head_stages(4096));
    CHECK(wpack_head_bytes(128256, 4096) * 16 == (size_t)128256 * 4096 * 2 * 13, "8B head: %zu bytes", wpack_head_bytes(128256, 4096));
    CHECK(wpack_head_stages(8192) == 64 && wpack_head_stages(264) == 3 && wpack_head_stages(8) == 1, "stage counts");
    if (!fails) printf("wpack_head_test: ok\n");
    return fails ? 1 : 0;
}
