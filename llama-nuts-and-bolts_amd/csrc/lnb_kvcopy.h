// lnb_kvcopy.h -- copy the KV rows [0, n_pos) of one context into other contexts (lnb_ctx_fork): the index arithmetic, plain C++ that compiles
// without HIP (tests/native/kvcopy_test.cpp runs exactly these functions on the host), and kv_fork_kernel, which walks them on the device.
//
// The unit of work is one 16-byte VECTOR = 8 bf16 values.  A cached layer is two arrays of kv_dim / 8 * capacity vectors:
//   K  [kv head][head_dim/8][capacity][8]  (lnb_device.h, GemvParams::cache_k): kv_dim/8 RUNS of n_pos vectors to copy; run r, position j is vector
//      r * capacity + j -- contexts of different capacities disagree on where every run starts;
//   V  [capacity][kv_dim]: the first n_pos * kv_dim / 8 vectors, the same index on both sides -- ONE run, whatever the capacities.
// So an array is (runs, run_len, stride): K = (kv_dim/8, n_pos, capacity), V = (1, n_pos * kv_dim/8, 0), and a vector is run * stride + j.
// A run is cut into TILES of KVC_TILE consecutive vectors; one workgroup of KVC_THREADS lanes takes a tile, lane t the vectors j0 + u * KVC_THREADS + t
// (u < KVC_UNROLL): every wave instruction touches 1 KB of consecutive memory.  The tile -> (run, j0) division is per tile, not per vector.
// Every offset is size_t: K of 64 KV heads of head_dim 128 at 131072 positions is 2^31 bytes (the last vector sits at 2^31 - 16, sixteen bytes
// short of what an int holds), and twice the heads put it at 2^32 - 16 -- a run index times a capacity times 16 must never pass through int.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define KVC_HD __host__ __device__ __forceinline__
#else
#define KVC_HD static inline
#endif

#define KVC_MAX_DST 128                 // LNB_MAX_FORK of include/lnb.h
#define KVC_VEC_BYTES 16
#define KVC_THREADS 256
#define KVC_UNROLL 4                    // independent 16-byte loads a lane has in flight before its store loop over the destinations
#define KVC_TILE (KVC_THREADS * KVC_UNROLL)
#define KVC_GRID_CAP 2048               // workgroups of a launch (256 CUs x 8): the rest is the grid-stride loop

// the runs of an array of a cached layer (which: 0 = K, 1 = V), their length in vectors and the distance between their starts in a context of `capacity`
KVC_HD size_t kvc_runs(int which, int kv_dim) { return which ? (size_t)1 : (size_t)(kv_dim >> 3); }
KVC_HD size_t kvc_run_len(int which, int kv_dim, int n_pos) { return which ? (size_t)n_pos * (size_t)(kv_dim >> 3) : (size_t)n_pos; }
KVC_HD size_t kvc_stride(int which, int capacity) { return which ? (size_t)0 : (size_t)capacity; }
// tiles of a run / of an array
KVC_HD size_t kvc_tiles_per_run(size_t run_len) { return (run_len + KVC_TILE - 1) / KVC_TILE; }
KVC_HD size_t kvc_tiles(int which, int kv_dim, int n_pos) { return kvc_runs(which, kv_dim) * kvc_tiles_per_run(kvc_run_len(which, kv_dim, n_pos)); }
// tile -> its run and the first vector of the tile inside the run
KVC_HD void kvc_tile_origin(size_t tile, size_t tiles_per_run, size_t* run, size_t* j0) { *run = tile / tiles_per_run; *j0 = (tile - *run * tiles_per_run) * KVC_TILE; }
// the vector lane `t` copies in step u of a tile that starts at j0 (valid while < run_len)
KVC_HD size_t kvc_lane_vec(size_t j0, int u, int t) { return j0 + (size_t)u * KVC_THREADS + (size_t)t; }
// vector index inside an array, and its byte offset
KVC_HD size_t kvc_vec_index(size_t run, size_t j, size_t stride) { return run * stride + j; }
KVC_HD size_t kvc_byte_offset(size_t vec) { return vec * KVC_VEC_BYTES; }
// bytes the rows [0, n_pos) of one cached layer take (K + V): what a fork moves per layer and destination, what a saved prefix holds per layer
KVC_HD size_t kvc_layer_bytes(int kv_dim, int n_pos) { return (size_t)2 * (size_t)n_pos * (size_t)kv_dim * 2; }
// destinations [*d0, *d1) of group z out of `groups` (grid.z; one group unless LNB_FORK_SPLIT asks for more: dealing the destinations over several
// groups, each of which reads the source again, measured 19 % faster at 128 positions into 16 contexts and 1 - 32 % slower in every other cell from 16 destinations on -- profiles/prefix_fork.md)
KVC_HD void kvc_group_range(int z, int groups, int n_dst, int* d0, int* d1) { *d0 = (int)((long long)z * n_dst / groups); *d1 = (int)((long long)(z + 1) * n_dst / groups); }

// The device table of one call, uploaded by lnb_ctx_fork: n_arrays = 2 * cached layers rows of (1 + n_dst) pointers -- [0] the source array, [1 + d]
// destination d's -- in the order K, V per cached layer, and the destinations' capacities.  Layers a stage keeps no cache for have no row.
struct KvForkTab {
    const void* const* ptrs;            // [n_arrays][1 + n_dst]
    const int* cap_dst;                 // [n_dst]
    int n_arrays, n_dst, kv_dim, n_pos, cap_src;
};

#if defined(__HIPCC__)
// One launch for every cached layer and every destination: grid.y = the array (K / V of a layer), grid.x strides over its tiles, grid.z = destination
// group.  A lane loads KVC_UNROLL vectors of the source (independent, all in flight), then stores them to each destination of its group; the
// destination's pointer and capacity are wave-uniform table reads.  No LDS, no atomics, vector stores only.  NT: non-temporal loads and stores (the
// source is read and every destination written exactly once) -- measured from 3 % faster to 20 % slower than the plain form, which wins 6 cells of 9 and is the default.
template <bool NT>
__global__ __launch_bounds__(KVC_THREADS) void kv_fork_kernel(KvForkTab tab) {
    typedef unsigned int kvc_u4 __attribute__((ext_vector_type(4)));
    const int a = (int)blockIdx.y, which = a & 1, t = (int)threadIdx.x;
    const size_t run_len = kvc_run_len(which, tab.kv_dim, tab.n_pos), tpr = kvc_tiles_per_run(run_len);
    const size_t tiles = kvc_runs(which, tab.kv_dim) * tpr, s_src = kvc_stride(which, tab.cap_src);
    const void* const* row = tab.ptrs + (size_t)a * (size_t)(1 + tab.n_dst);
    const kvc_u4* src = (const kvc_u4*)row[0];
    int d0, d1;
    kvc_group_range((int)blockIdx.z, (int)gridDim.z, tab.n_dst, &d0, &d1);
    for (size_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        size_t run, j0;
        kvc_tile_origin(tile, tpr, &run, &j0);
        kvc_u4 x[KVC_UNROLL];
#pragma unroll
        for (int u = 0; u < KVC_UNROLL; u++) {
            const size_t j = kvc_lane_vec(j0, u, t);
            if (j < run_len) { const kvc_u4* p = src + kvc_vec_index(run, j, s_src); x[u] = NT ? __builtin_nontemporal_load(p) : *p; }
        }
        for (int d = d0; d < d1; d++) {
            kvc_u4* dst = (kvc_u4*)row[1 + d];
            const size_t s_dst = kvc_stride(which, tab.cap_dst[d]);
#pragma unroll
            for (int u = 0; u < KVC_UNROLL; u++) {
                const size_t j = kvc_lane_vec(j0, u, t);
                if (j < run_len) { kvc_u4* p = dst + kvc_vec_index(run, j, s_dst); if (NT) __builtin_nontemporal_store(x[u], p); else *p = x[u]; }
            }
        }
    }
}
#endif
