// lnb_wpack.h -- the lossless 13-bit planar copy of a bf16 weight matrix that the one-token gate|up kernel and the one-token LM head stream instead of
// the raw bf16 (gemv_chain_kernel's packed source form).  Plain C++ shared by host and device: tests/native/wpack_test.cpp and wpack_head_test.cpp include exactly this file.
//
// bf16 = sign | 8 exponent bits | 7 mantissa bits.  The LOW byte (exponent bit 0 + mantissa) is kept raw.  The HIGH byte is sign | exponent >> 1,
// and the non-zero weights of a matrix live in a few dozen binades, so exponent >> 1 is stored as a 4-bit code relative to a per-matrix window:
//   base   = (smallest exponent >> 1 over the weights with exponent >= 2) - 1      (an all-zero matrix: base 0)
//   code 0 : exponent >> 1 == 0 -- with the refusals below that is +-0 only
//   code c : exponent >> 1 == base + c, c = 1..15                                   (30 binades of non-zero weights)
// A matrix with a subnormal, an exponent of 1, an Inf / NaN or a non-zero weight above the window is NOT packable (wpack_window says why): it keeps
// the raw path.  That is a decision per matrix when the copy is built, never per element at run time.
//
// A GROUP is 32 weights w[0..31], what one helper lane converts per stage; quad g = 0..7 is w[4g .. 4g+3], unit u = 0..3 is quads 2u and 2u+1 (one
// 16-byte unit of the resident chain layout).  52 bytes instead of 64:
//   low plane   8 dwords: dword g, byte j          = w[4g + j] & 0xFF
//   code plane  4 dwords: dword u, byte j          = code(w[8u + j]) | code(w[8u + 4 + j]) << 4     -> N & 0x0F0F0F0F and (N >> 4) & 0x0F0F0F0F are a
//                                                     quad's four codes, one per byte
//   sign plane  1 dword : bit 8j + 7 - g           = sign(w[4g + j])                                -> (S << g) & 0x80808080 is quad g's signs in place
// The four high bytes of a quad are then made together (wpack_hi4) and each weight is widened to f32 by one byte permute (wpack_wide).
#pragma once
#include <stdint.h>
#include <stddef.h>

#if defined(__HIPCC__)
#define LNB_WP_HD __host__ __device__ __forceinline__
#else
#define LNB_WP_HD static inline
#endif

#define WPACK_GROUP 32                   // weights per group
#define WPACK_GROUP_BYTES 52             // 32 + 16 + 4
enum { WPACK_OK = 0, WPACK_SUBNORMAL = 1, WPACK_INFNAN = 2, WPACK_WINDOW = 3, WPACK_NOMEM = 4 };   // (4: the copy could not be allocated -- host side only)

// ---- the window ---------------------------------------------------------------------------------
// what a pass over a matrix collects (the device reduces the same four words with atomics)
struct WpackStats { uint32_t min_e2, max_e2, subnormal, infnan; };      // e2 = exponent >> 1 over the weights with 2 <= exponent <= 254
LNB_WP_HD void wpack_stats_init(WpackStats* s) { s->min_e2 = 0xFFu; s->max_e2 = 0; s->subnormal = 0; s->infnan = 0; }
LNB_WP_HD void wpack_stats_add(WpackStats* s, uint16_t w) {
    const uint32_t e = (w >> 7) & 0xFFu;
    if (e == 0xFFu) { s->infnan = 1; return; }
    if (e < 2) { if (w & 0x7FFFu) s->subnormal = 1; return; }            // +-0 is fine; a subnormal or an exponent of 1 is not
    const uint32_t e2 = e >> 1;
    if (e2 < s->min_e2) s->min_e2 = e2;
    if (e2 > s->max_e2) s->max_e2 = e2;
}
// -> WPACK_OK and *base, or the reason the matrix keeps the raw path
LNB_WP_HD int wpack_window(const WpackStats* s, uint32_t* base) {
    *base = 0;
    if (s->subnormal) return WPACK_SUBNORMAL;
    if (s->infnan) return WPACK_INFNAN;
    if (s->max_e2 == 0) return WPACK_OK;                                 // nothing but zeros
    *base = s->min_e2 - 1;
    return s->max_e2 - *base <= 15 ? WPACK_OK : WPACK_WINDOW;
}

// ---- the scalar definition ----------------------------------------------------------------------
LNB_WP_HD uint32_t wpack_code(uint16_t w, uint32_t base) { const uint32_t e2 = (w >> 8) & 0x7Fu; return e2 ? e2 - base : 0; }
LNB_WP_HD uint16_t wpack_scalar(uint32_t code, uint32_t sign, uint32_t low, uint32_t base) {
    return (uint16_t)((sign << 15) | ((code ? base + code : 0u) << 8) | low);
}
// one group: 32 weights -> 8 + 4 + 1 dwords (the matrix must have passed wpack_window with this base)
LNB_WP_HD void wpack_pack_group(const uint16_t* w, uint32_t base, uint32_t* low8, uint32_t* code4, uint32_t* sign1) {
    for (int g = 0; g < 8; g++) low8[g] = 0;
    for (int u = 0; u < 4; u++) code4[u] = 0;
    uint32_t s = 0;
    for (int g = 0; g < 8; g++)
        for (int j = 0; j < 4; j++) {
            const uint16_t v = w[4 * g + j];
            low8[g] |= (uint32_t)(v & 0xFFu) << (8 * j);
            code4[g >> 1] |= wpack_code(v, base) << (8 * j + 4 * (g & 1));
            s |= (uint32_t)(v >> 15) << (8 * j + 7 - g);
        }
    *sign1 = s;
}
LNB_WP_HD void wpack_unpack_group(const uint32_t* low8, const uint32_t* code4, uint32_t sign1, uint32_t base, uint16_t* w) {
    for (int g = 0; g < 8; g++)
        for (int j = 0; j < 4; j++)
            w[4 * g + j] = wpack_scalar((code4[g >> 1] >> (8 * j + 4 * (g & 1))) & 0xFu, (sign1 >> (8 * j + 7 - g)) & 1u, (low8[g] >> (8 * j)) & 0xFFu, base);
}

// ---- the decode the kernel runs: four weights at a time, no per-element extraction ----------------
// the four codes of quad g = 2u + h, one per byte
LNB_WP_HD uint32_t wpack_spread(uint32_t code_dword, int h) { return (h ? code_dword >> 4 : code_dword) & 0x0F0F0F0Fu; }
// the four high bytes of a quad: base + code where the code is not 0 (no byte carries: code <= 15, base + code <= 127), signs OR-ed in.
// base4 = base * 0x01010101
LNB_WP_HD uint32_t wpack_hi4(uint32_t c, uint32_t signs, int g, uint32_t base4) {
    const uint32_t nz = (c + 0x7F7F7F7Fu) & 0x80808080u;                 // bit 7 of a byte: its code is not 0
    const uint32_t keep = nz - (nz >> 7);                                // 0x7F in those bytes
    return ((c + base4) & keep) | ((signs << g) & 0x80808080u);
}
// weight j of the quad as the f32 bit pattern of its bf16: high byte, low byte, two zero bytes -- one v_perm_b32 on the device
template <int J> LNB_WP_HD uint32_t wpack_wide(uint32_t hi4, uint32_t lo4) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(hi4, lo4, ((4u + J) << 24) | ((uint32_t)J << 16) | 0x0C0Cu);
#else
    return (((hi4 >> (8 * J)) & 0xFFu) << 24) | (((lo4 >> (8 * J)) & 0xFFu) << 16);
#endif
}

// ---- the stream ---------------------------------------------------------------------------------
// A STAGE of the packed gate|up stream is one group per helper lane, plane by plane so that every load of a wave is one contiguous run:
//   [lanes x 16 B low plane, quads 0..3][lanes x 16 B low plane, quads 4..7][lanes x 16 B code plane][lanes x 4 B sign plane]
// Lane L of a stage holds the two (8-wide k chunk, row) pairs pq = L and pq = lanes + L of the stage: kc = pq / RW, r = pq % RW (lanes * 2 = RW * chunks per
// stage); unit 2 pi + c of its group is chain c (0 gate, 1 up) of pair pi -- the unit ((kc_global * 2 + c) * RW + r) of the block's resident chain
// layout.  A block is a whole number of stages: the chunks past K are zeros (code 0).
LNB_WP_HD size_t wpack_stage_bytes(int lanes) { return (size_t)lanes * WPACK_GROUP_BYTES; }
LNB_WP_HD int wpack_stages(int K, int lanes, int rw) { const int kcs = 2 * lanes / rw; return ((K >> 3) + kcs - 1) / kcs; }
LNB_WP_HD size_t wpack_bytes(int n_blocks, int K, int lanes, int rw) { return (size_t)n_blocks * (size_t)wpack_stages(K, lanes, rw) * wpack_stage_bytes(lanes); }
// where lane L's planes of a stage lie behind the stage's first byte: plane 0 low bytes of quads 0..3, 1 low bytes of quads 4..7, 2 codes (16 bytes each), 3 signs (4 bytes)
LNB_WP_HD size_t wpack_plane_off(int lanes, int plane, int L) { return (size_t)lanes * 16 * plane + (size_t)L * (plane == 3 ? 4 : 16); }

// ---- the LM head's stream ------------------------------------------------------------------------
// The head keeps its resident layout [N/64][K/8][1][64][8] (one chain per lane: prefill, batches, every other path).  Its packed copy is cut for a TWO-chain
// kernel instead: a block is 128 vocabulary rows, chain 0 = row 128 b + r, chain 1 = row 128 b + 64 + r (r = 0..63) -- the resident blocks 2 b and 2 b + 1 --
// streamed by 512 helper lanes in stages of 16 chunks (128 k steps).  Stage, plane and pair arithmetic are the gate|up stream's with RW = 64; only the source
// of a unit differs.  Rows at or beyond N and chunks at or beyond K / 8 are zeros (code 0).
#define WPACK_HEAD_LANES 512
#define WPACK_HEAD_RW 64                  // rows per chain of a block
LNB_WP_HD int wpack_head_blocks(int N) { return (N + 2 * WPACK_HEAD_RW - 1) / (2 * WPACK_HEAD_RW); }
LNB_WP_HD int wpack_head_stages(int K) { return wpack_stages(K, WPACK_HEAD_LANES, WPACK_HEAD_RW); }
LNB_WP_HD size_t wpack_head_bytes(int N, int K) { return wpack_bytes(wpack_head_blocks(N), K, WPACK_HEAD_LANES, WPACK_HEAD_RW); }
// first byte of (block b, stage st) in the copy
LNB_WP_HD size_t wpack_head_stage_off(int K, int b, int st) { return ((size_t)b * (size_t)wpack_head_stages(K) + (size_t)st) * wpack_stage_bytes(WPACK_HEAD_LANES); }
// unit u = 0..3 of the group of (block b, stage st, lane L): the 16-byte unit of the resident layout it holds (an index in units), or -1: zeros
LNB_WP_HD long long wpack_head_src_unit(int N, int K, int b, int st, int L, int u) {
    const int kcs = 2 * WPACK_HEAD_LANES / WPACK_HEAD_RW;                  // chunks per stage
    const int pq = (u >> 1) * WPACK_HEAD_LANES + L, kc = st * kcs + pq / WPACK_HEAD_RW, r = pq % WPACK_HEAD_RW, rb = 2 * b + (u & 1);
    if (kc >= (K >> 3) || rb * WPACK_HEAD_RW + r >= N) return -1;
    return ((long long)rb * (K >> 3) + kc) * WPACK_HEAD_RW + r;
}
