// kvcopy_test.cpp -- the index arithmetic of csrc/lnb_kvcopy.h on the host (tests/test_prefix_fork_cpu.py builds it with -fsanitize=address,undefined).
// It walks the header's functions exactly as kv_fork_kernel does -- array, destination group, grid-stride tile loop, lane, unroll step -- over plain host
// arrays in the device layout, several destinations of different capacities at once, and reads the result back through lnb_ctx_read_kv's formula:
// rows below n_pos must be the source's, every other element of a destination must keep its sentinel, the source must be untouched.  An out-of-range
// index is a heap overflow the sanitizer reports.  The last part checks offsets alone at geometries whose arrays reach and pass 2^31 bytes.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../llama-nuts-and-bolts_amd/csrc/lnb_kvcopy.h"

static int g_bad = 0;
#define CHECK(c, ...) do { if (!(c)) { if (g_bad++ < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

struct Vec { unsigned char b[KVC_VEC_BYTES]; };
static const uint16_t SENTINEL = 0xDEAD;

// element (position j, kv head kh, dim d) of K in a context of capacity SL: lnb_ctx_read_kv's formula; of V: [position][kv_dim]
static size_t k_elem(int hd, int SL, int j, int kh, int d) { const int nk = hd >> 3; return (((size_t)kh * nk + (d >> 3)) * SL + j) * 8 + (d & 7); }
static size_t v_elem(int kv_dim, int hd, int j, int kh, int d) { return (size_t)j * kv_dim + (size_t)kh * hd + d; }
// a value per (position, kv head, d): 40503 is odd, so the map is one-to-one on 16 bits -- distinct wherever capacity * kv_dim <= 65536 (every listed
// shape; the extra multi-tile shape repeats every 512 positions, far beyond any stride it could confuse).  K and V differ.
static uint16_t value(int which, int kv_dim, int hd, int j, int kh, int d) { return (uint16_t)((((uint32_t)j * kv_dim + kh * hd + d) * 40503u + (which ? 12345u : 0u)) & 0xFFFFu); }

// kv_fork_kernel on the host: grid (gx, 2, gz), KVC_THREADS lanes, the same header calls in the same order
static void fork_on_host(const KvForkTab& tab, int gx, int gz) {
    for (int a = 0; a < tab.n_arrays; a++) {
        const int which = a & 1;
        const size_t run_len = kvc_run_len(which, tab.kv_dim, tab.n_pos), tpr = kvc_tiles_per_run(run_len);
        const size_t tiles = kvc_runs(which, tab.kv_dim) * tpr, s_src = kvc_stride(which, tab.cap_src);
        const void* const* row = tab.ptrs + (size_t)a * (size_t)(1 + tab.n_dst);
        const Vec* src = (const Vec*)row[0];
        for (int z = 0; z < gz; z++) {
            int d0, d1;
            kvc_group_range(z, gz, tab.n_dst, &d0, &d1);
            for (int bx = 0; bx < gx; bx++)
                for (size_t tile = (size_t)bx; tile < tiles; tile += (size_t)gx) {
                    size_t run, j0;
                    kvc_tile_origin(tile, tpr, &run, &j0);
                    for (int t = 0; t < KVC_THREADS; t++) {
                        Vec x[KVC_UNROLL];
                        for (int u = 0; u < KVC_UNROLL; u++) {
                            const size_t j = kvc_lane_vec(j0, u, t);
                            if (j < run_len) x[u] = src[kvc_vec_index(run, j, s_src)];
                        }
                        for (int d = d0; d < d1; d++) {
                            Vec* dst = (Vec*)row[1 + d];
                            const size_t s_dst = kvc_stride(which, tab.cap_dst[d]);
                            for (int u = 0; u < KVC_UNROLL; u++) {
                                const size_t j = kvc_lane_vec(j0, u, t);
                                if (j < run_len) dst[kvc_vec_index(run, j, s_dst)] = x[u];
                            }
                        }
                    }
                }
        }
    }
}

static void run_shape(int hd, int KVH, int SLs, int SLd, int n_pos) {
    const int kv_dim = KVH * hd;
    const int caps[3] = {SLd, SLd + 5, n_pos};                  // several destinations at once: the listed capacity, an odd one, the tightest one
    const int n_dst = 3;
    std::vector<uint16_t> sk((size_t)SLs * kv_dim), sv((size_t)SLs * kv_dim);
    for (int j = 0; j < SLs; j++)
        for (int kh = 0; kh < KVH; kh++)
            for (int d = 0; d < hd; d++) {
                sk[k_elem(hd, SLs, j, kh, d)] = value(0, kv_dim, hd, j, kh, d);
                sv[v_elem(kv_dim, hd, j, kh, d)] = value(1, kv_dim, hd, j, kh, d);
            }
    const std::vector<uint16_t> sk0 = sk, sv0 = sv;
    std::vector<std::vector<uint16_t>> dk(n_dst), dv(n_dst);
    for (int i = 0; i < n_dst; i++) { dk[i].assign((size_t)caps[i] * kv_dim, SENTINEL); dv[i].assign((size_t)caps[i] * kv_dim, SENTINEL); }
    std::vector<const void*> ptrs;
    ptrs.push_back(sk.data()); for (int i = 0; i < n_dst; i++) ptrs.push_back(dk[i].data());
    ptrs.push_back(sv.data()); for (int i = 0; i < n_dst; i++) ptrs.push_back(dv[i].data());
    KvForkTab tab;
    tab.ptrs = ptrs.data(); tab.cap_dst = caps; tab.n_arrays = 2; tab.n_dst = n_dst; tab.kv_dim = kv_dim; tab.n_pos = n_pos; tab.cap_src = SLs;
    CHECK(kvc_layer_bytes(kv_dim, n_pos) == (size_t)4 * n_pos * kv_dim, "layer bytes");
    fork_on_host(tab, 3, 2);                                     // three blocks stride the tiles, the destinations in two groups (2 + 1)
    CHECK(sk == sk0 && sv == sv0, "hd %d (%d, %d, %d): the source changed", hd, SLs, SLd, n_pos);
    for (int i = 0; i < n_dst; i++) {
        std::vector<uint16_t> ek((size_t)caps[i] * kv_dim, SENTINEL), ev((size_t)caps[i] * kv_dim, SENTINEL);
        for (int j = 0; j < n_pos; j++)
            for (int kh = 0; kh < KVH; kh++)
                for (int d = 0; d < hd; d++) {
                    ek[k_elem(hd, caps[i], j, kh, d)] = sk0[k_elem(hd, SLs, j, kh, d)];
                    ev[v_elem(kv_dim, hd, j, kh, d)] = sv0[v_elem(kv_dim, hd, j, kh, d)];
                }
        CHECK(dk[i] == ek, "hd %d (%d, %d, %d): K of destination %d (capacity %d)", hd, SLs, SLd, n_pos, i, caps[i]);
        CHECK(dv[i] == ev, "hd %d (%d, %d, %d): V of destination %d (capacity %d)", hd, SLs, SLd, n_pos, i, caps[i]);
    }
}

// offsets only: the last vector a launch would touch in K of a context of `cap` positions with KVH heads of head_dim hd, against 64-bit arithmetic
// written out independently of the header
static uint64_t last_k_offset(int KVH, int hd, int cap) {
    const int kv_dim = KVH * hd;
    const size_t run_len = kvc_run_len(0, kv_dim, cap), tpr = kvc_tiles_per_run(run_len), tiles = kvc_tiles(0, kv_dim, cap);
    size_t run, j0;
    kvc_tile_origin(tiles - 1, tpr, &run, &j0);
    size_t j = 0;
    for (int u = 0; u < KVC_UNROLL; u++) { const size_t c = kvc_lane_vec(j0, u, KVC_THREADS - 1); if (c < run_len) j = c; }
    const uint64_t got = kvc_byte_offset(kvc_vec_index(run, j, kvc_stride(0, cap)));
    const uint64_t want = ((uint64_t)KVH * (uint64_t)(hd / 8) * (uint64_t)cap - 1u) * 16u;
    CHECK(got == want, "last K offset of %d heads: %llu, expected %llu", KVH, (unsigned long long)got, (unsigned long long)want);
    const uint64_t v_got = kvc_byte_offset(kvc_vec_index(0, kvc_run_len(1, kv_dim, cap) - 1, kvc_stride(1, cap)));
    CHECK(v_got == want, "last V offset of %d heads: %llu, expected %llu", KVH, (unsigned long long)v_got, (unsigned long long)want);
    return got;
}

int main() {
    static_assert(sizeof(Vec) == KVC_VEC_BYTES && sizeof(size_t) == 8, "16-byte vectors, 64-bit offsets");
    const int shapes[5][3] = {{7, 7, 7}, {64, 41, 37}, {41, 300, 37}, {96, 96, 1}, {300, 64, 64}};
    const int geo[3][2] = {{32, 4}, {64, 2}, {128, 1}};          // head_dim, KV heads (kv_dim 128: values distinct up to 512 positions)
    for (auto& g : geo)
        for (auto& s : shapes) run_shape(g[0], g[1], s[0], s[1], s[2]);
    run_shape(64, 2, 2100, 1500, 1300);                          // K runs of more than one tile, the second one partial
    run_shape(128, 3, 41, 64, 37);                               // an odd number of KV heads
    // 64 KV heads of head_dim 128 at 131072 positions: K is exactly 2^31 bytes, so its last vector starts at 2^31 - 16 -- the largest offset this geometry
    // has, sixteen bytes short of overflowing an int.  Twice and four times the heads pass 2^31 and 2^32.
    const uint64_t o64 = last_k_offset(64, 128, 131072), o128 = last_k_offset(128, 128, 131072), o256 = last_k_offset(256, 128, 131072);
    CHECK(o64 == (1ull << 31) - 16, "64 heads: %llu", (unsigned long long)o64);
    CHECK(o128 == (1ull << 32) - 16 && o128 > (1ull << 31), "128 heads: %llu", (unsigned long long)o128);
    CHECK(o256 == (1ull << 33) - 16 && o256 > (1ull << 32), "256 heads: %llu", (unsigned long long)o256);
    // destination groups: every destination in exactly one group, no group empty
    for (int n = 1; n <= KVC_MAX_DST; n++)
        for (int g = 1; g <= n; g++) {
            int next = 0;
            for (int z = 0; z < g; z++) { int d0, d1; kvc_group_range(z, g, n, &d0, &d1); CHECK(d0 == next && d1 > d0, "group %d of %d (%d destinations)", z, g, n); next = d1; }
            CHECK(next == n, "%d groups of %d destinations end at %d", g, n, next);
        }
    if (g_bad) { printf("kvcopy_test: %d failure(s)\n", g_bad); return 1; }
    printf("kvcopy_test: ok\n");
    return 0;
}
