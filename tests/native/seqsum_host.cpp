// Host harness for csrc/lnb_seqsum.h: emulates the 64-lane device algorithm with loops so the exact-parallel
// sequential sum can be fuzzed against the plain sequential f32 loop on the CPU (tests/test_seqsum.py).
// build: g++ -O2 -ffp-contract=off -shared -fPIC tests/native/seqsum_host.cpp -o tests/native/libseqsum_host.so
#include "../../llama-nuts-and-bolts_amd/csrc/lnb_seqsum.h"
#include <vector>

extern "C" float seqsum_ref(const float* p, int K) {
    float s = 0.0f;
    for (int k = 0; k < K; k++) s += p[k];
    return s;
}

// same structure as rms_scale_scan() in lnb_kernels.hip: nb blocks of bs = K/nb terms
extern "C" float seqsum_scan(const float* p, int K, int nb, int* n_fast_out) {
    const int bs = K / nb;
    std::vector<float> P(nb), S(nb + 1);
    for (int l = 0; l < nb; l++) { float a = 0.0f; for (int i = 0; i < bs; i++) a += p[l * bs + i]; P[l] = a; }
    S[0] = 0.0f;
    for (int l = 0; l < nb; l++) S[l + 1] = S[l] + P[l];          // (device: wave prefix scan; any order is fine, it is only a guess)
    std::vector<SeqBlock> B(nb);
    for (int l = 0; l < nb; l++) {
        SeqBlock b; b.c0 = 0; b.c1 = 0; b.e = seq_guess(S[l], S[l + 1]); b.ok = b.e != 0;
        if (b.ok) for (int i = 0; i < bs; i++) { seq_step(b, p[l * bs + i]); if ((uint32_t)b.c0 > 0x2000000u || (uint32_t)b.c1 > 0x2000000u) b.ok = 0; }
        B[l] = b;
    }
    float s = 0.0f; int fast = 0;
    for (int l = 0; l < nb; l++) {
        if (seq_apply(s, B[l])) { fast++; continue; }
        for (int i = 0; i < bs; i++) s += p[l * bs + i];
    }
    if (n_fast_out) *n_fast_out = fast;
    return s;
}


// ---- the multi-wave form (rms_fold / rms_scale_wide in lnb_kernels.hip), emulated lane by lane -------------------------
// NH folding waves of 64 lanes; lane = one leaf of LEAF = seq_leaf_size(K, NH*64) terms (zero padded past K).  Per wave
// ("heap" of 64 leaves) a segmented inclusive scan composes the leaf maps of every run of equal-binade valid leaves; the
// walker adds the first `head` terms one by one, then visits only the run ends and the invalid leaves (item mask),
// applying the run's composed map when it starts exactly at the walker's position and verifies, else replaying the
// leaves' terms.  Returns the sum; *visits = items visited, *raw = leaves replayed.
static long leaf_mismatch = 0;
extern "C" long seqsum_leaf_mismatches() { return leaf_mismatch; }
extern "C" float seqsum_tree(const float* pin, int K, int NH, int head_terms, int* visits, int* raw) {
    const int LEAF = seq_leaf_size(K, NH * 64), nleaf = (K + LEAF - 1) / LEAF, TB = NH * 64;
    std::vector<float> pv((size_t)TB * LEAF + 64, 0.0f);
    for (int k = 0; k < K; k++) pv[k] = pin[k];
    const float* p = pv.data();
    std::vector<float> bs(TB, 0.0f), lo(TB), hi(TB);
    for (int b = 0; b < nleaf; b++) {
        const float* q = p + (size_t)b * LEAF;
        float v = 0.0f;
        for (int i = 0; i < LEAF; i += 4) v += (q[i] + q[i + 1]) + (q[i + 2] + q[i + 3]);       // (only a guess: any order)
        bs[b] = v;
    }
    float run = 0.0f;                                                      // approximate prefix: wave scans + wave totals
    for (int g = 0; g < NH; g++) {
        float incl = 0.0f;
        for (int l = 0; l < 64; l++) { const int b = g * 64 + l; lo[b] = run + incl; incl += bs[b]; hi[b] = run + incl; }
        run += incl;
    }
    int head = head_terms < K ? head_terms : K;
    const int headleaf = head / LEAF;
    head = headleaf * LEAF;
    std::vector<SeqNode> rec((size_t)TB);
    std::vector<uint64_t> items(NH);
    std::vector<int> scan_failed(NH, 0);
    for (int g = 0; g < NH; g++) {
        SeqNode n[64]; int f[64], st[64];
        for (int l = 0; l < 64; l++) {
            const int b = g * 64 + l;
            n[l].a = 0; n[l].b = 0;
            if (b < nleaf) {
                n[l] = seq_leaf(p + (size_t)b * LEAF, LEAF, lo[b], hi[b]);
                // the two-sums evaluation (device path) against the integer one, term by term: same node whenever the integer one is valid;
                // where only the simulated one is valid (it may accept what the conservative integer test rejects) the walk still verifies it
                const SeqNode chk = seq_leaf_steps(p + (size_t)b * LEAF, LEAF, lo[b], hi[b]);
                if ((chk.a >> 24) && (chk.a != n[l].a || chk.b != n[l].b)) leaf_mismatch++;
            }
            if (b < nleaf && bs[b] == 0.0f && !(n[l].a >> 24)) n[l].a = SEQ_ZERO_LEAF;
        }
        for (int l = 0; l < 64; l++) f[l] = seq_is_start(l, n[l], l ? n[l - 1] : n[l], g * 64 + l == headleaf);
        uint64_t mask = 0;
        for (int l = 0; l < 64; l++) if (!(n[l].a >> 24) || l == 63 || f[l + 1]) mask |= 1ull << l;
        for (int l = 0; l < 64; l++) st[l] = l;
        for (int d = 1; d < 64; d <<= 1) {                                 // Hillis-Steele, all lanes in lock step
            SeqNode nn[64]; int ff[64], ss[64];
            for (int l = 0; l < 64; l++) {
                nn[l] = n[l]; ff[l] = f[l]; ss[l] = st[l];
                if (l >= d && !f[l]) scan_failed[g] |= !seq_scan_step(nn[l], ff[l], ss[l], n[l - d], f[l - d], st[l - d]);
            }
            for (int l = 0; l < 64; l++) { n[l] = nn[l]; f[l] = ff[l]; st[l] = ss[l]; }
        }
        for (int l = 0; l < 64; l++) { rec[(size_t)g * 64 + l].a = n[l].a; rec[(size_t)g * 64 + l].b = n[l].b | ((uint32_t)st[l] << 24); }
        items[g] = mask;
    }
    int nv = 0, nr = 0;
    float s = 0.0f;
    for (int k = 0; k < head; k++) s += p[k];
    uint32_t sb = seq_f2u(s);
    for (int g = 0; g < NH; g++) {
        int nloc = nleaf - g * 64; nloc = nloc < 0 ? 0 : (nloc > 64 ? 64 : nloc);
        int pos = headleaf - g * 64; pos = pos < 0 ? 0 : pos;
        uint64_t mask = items[g], zm = 0;
        for (int l = 0; l < 64; l++) if (rec[(size_t)g * 64 + l].a == SEQ_ZERO_LEAF) zm |= 1ull << l;
        mask &= ~zm;                                                       // leaves of exact zeros: stepped over, not visited
        while (mask) {
            const int i = __builtin_ctzll(mask); mask &= mask - 1;
            if (i < pos) continue;
            if (i >= nloc) break;
            nv++;
            SeqNode n = rec[(size_t)g * 64 + i];
            int st = (int)(n.b >> 24); n.b &= 0xFFFFFFu;
            // rms_walk_fast (lnb_kernels.hip): the items tile the leaves by construction unless a composition of the scan failed, so the
            // record's start is only checked then (rms_walk_heap); a replay starts behind the previous item either way
            if (!scan_failed[g]) st = pos;
            else if (st > pos && ((((1ull << st) - 1ull) & (~0ull << pos)) & ~zm) == 0ull) pos = st;   // zeros: nothing to add
            if (!(st == pos && seq_apply_node(sb, n))) {
                float f = seq_u2f(sb);
                for (int l = pos; l <= i; l++) { const float* q = p + ((size_t)g * 64 + l) * LEAF; for (int t = 0; t < LEAF; t++) f += q[t]; nr++; }
                sb = seq_f2u(f);
            }
            pos = i + 1;
        }
    }
    if (visits) *visits = nv;
    if (raw) *raw = nr;
    return seq_u2f(sb);
}


// ---- the branch-free walk over a row's ITEM LIST (rms_fold's emission + rms_scale_wide), emulated lane by lane as the device runs it --------
// Same leaves as seqsum_tree; what differs from it follows the kernels line by line:
//   * the approximate prefix: a leaf's tree sum in rms_tree16 order per 16 terms, the wave's inclusive sum in wave_inclusive_sum's DPP order (in-row shifts by
//     1, 2, 4, 8, then lane 15 into rows 1 and 3, then lane 31 into rows 2 and 3), the waves in front added one by one;
//   * binades guessed with the tight margin; a leaf that crosses a binade edge is split (seq_split_leaf); the segmented scan in the device's six steps;
//   * items in leaf order per wave: the end of every run, the two items of every split leaf, LEAF single-term items for an uncovered leaf whose TREE SUM is
//     finite; leaves of exact zeros emit nothing; a wave whose items exceed its 128-entry list segment, or with a leaf nothing covers, flags the row;
//   * the walker: every item applied unconditionally, the checks OR-ed; a flagged row, one with more than 64 items or with a failed check takes the record
//     walk (rms_walk_fast; rms_walk_heap for a wave whose scan failed) over the SAME records.
// *path = the device's path word (RMS_PATH_*, lnb_seqsum.h), *n_items = the list's length.
static float tree16(const float* tv) {
    return (((tv[0] + tv[1]) + (tv[2] + tv[3])) + ((tv[4] + tv[5]) + (tv[6] + tv[7]))) + (((tv[8] + tv[9]) + (tv[10] + tv[11])) + ((tv[12] + tv[13]) + (tv[14] + tv[15])));
}
static int dbg_reason = 0;
extern "C" int seqsum_dbg_reason() { return dbg_reason; }
extern "C" float seqsum_device(const float* pin, int K, int NH, int head_terms, uint32_t* path_out, int* n_items) {
    const int LEAF = seq_leaf_size(K, NH * 64), nleaf = (K + LEAF - 1) / LEAF, TB = NH * 64;
    std::vector<float> pv((size_t)TB * LEAF + 64, 0.0f);
    for (int k = 0; k < K; k++) pv[k] = pin[k];
    const float* p = pv.data();
    std::vector<float> bs(TB, 0.0f), incl(TB, 0.0f), lo(TB), hi(TB), wtot(NH);
    for (int b = 0; b < nleaf; b++) {
        const float* q = p + (size_t)b * LEAF;
        float v = 0.0f;
        for (int c = 0; c < LEAF; c += 16) {
            float tv[16];
            for (int i = 0; i < 16; i++) tv[i] = c + (i & ~3) < LEAF ? q[c + i] : 0.0f;
            v = c ? v + tree16(tv) : tree16(tv);
        }
        bs[b] = v;
    }
    for (int g = 0; g < NH; g++) {                                         // wave_inclusive_sum
        float v[64], o[64];
        for (int l = 0; l < 64; l++) v[l] = bs[g * 64 + l];
        for (int d = 1; d < 16; d <<= 1) { for (int l = 0; l < 64; l++) o[l] = (l & 15) >= d ? v[l - d] : 0.0f; for (int l = 0; l < 64; l++) v[l] += o[l]; }
        for (int l = 0; l < 64; l++) o[l] = (l & 16) ? v[(l & ~15) - 1] : 0.0f;
        for (int l = 0; l < 64; l++) v[l] += o[l];
        for (int l = 0; l < 64; l++) o[l] = l >= 32 ? v[31] : 0.0f;
        for (int l = 0; l < 64; l++) v[l] += o[l];
        for (int l = 0; l < 64; l++) incl[g * 64 + l] = v[l];
        wtot[g] = v[63];
    }
    for (int g = 0; g < NH; g++) {
        float base = 0.0f;
        for (int w = 0; w < NH; w++) base += w < g ? wtot[w] : 0.0f;
        for (int l = 0; l < 64; l++) { const int b = g * 64 + l; lo[b] = base + (incl[b] - bs[b]); hi[b] = base + incl[b]; }
    }
    int head = head_terms < K ? head_terms : K;
    const int headleaf = head / LEAF;
    head = headleaf * LEAF;
    std::vector<SeqNode> rec((size_t)TB);
    std::vector<uint64_t> items(NH);
    std::vector<int> scan_failed(NH, 0), cntw(NH, 0), flag(NH, 0);
    std::vector<std::vector<SeqItem>> seg(NH);
    dbg_reason = 0;
    for (int g = 0; g < NH; g++) {
        SeqNode n[64]; int f[64], st[64]; SeqSplit sp[64]; bool split_ok[64];
        for (int l = 0; l < 64; l++) {
            const int b = g * 64 + l;
            n[l].a = 0; n[l].b = 0; sp[l].ok = 0; split_ok[l] = false;
            if (b < nleaf) {
                const int32_t e = seq_guess_tight(lo[b], hi[b]);
                float s0, s1; seq_sim_init(e, s0, s1);
                for (int i = 0; i < LEAF; i++) { s0 = s0 + p[(size_t)b * LEAF + i]; s1 = s1 + p[(size_t)b * LEAF + i]; }
                n[l] = seq_sim_node(e, s0, s1);
                if (bs[b] == 0.0f && !(n[l].a >> 24)) n[l].a = SEQ_ZERO_LEAF;
                if (!(n[l].a >> 24) && n[l].a != SEQ_ZERO_LEAF && seq_split_candidate(lo[b], hi[b])) { sp[l] = seq_split_leaf(p + (size_t)b * LEAF, LEAF, lo[b], hi[b]); split_ok[l] = sp[l].ok != 0; }
            }
        }
        SeqNode none; none.a = 0; none.b = 0;
        for (int l = 0; l < 64; l++) f[l] = seq_is_start(l, n[l], l ? n[l - 1] : none, g * 64 + l == headleaf);
        uint64_t mask = 0;
        for (int l = 0; l < 64; l++) if (!(n[l].a >> 24) || l == 63 || f[l + 1 < 64 ? l + 1 : 63]) mask |= 1ull << l;
        for (int l = 0; l < 64; l++) st[l] = l;
        int failed = 0;
        for (int step = 0; step < 6; step++) {                             // the six DPP steps of the segmented scan, all lanes in lock step
            SeqNode nn[64]; int ff[64], ss[64];
            for (int l = 0; l < 64; l++) {
                nn[l] = n[l]; ff[l] = f[l]; ss[l] = st[l];
                int src = -1;
                if (step < 4) { const int d = 1 << step; if ((l & 15) >= d) src = l - d; }
                else if (step == 4) { if (l & 16) src = (l & ~15) - 1; }
                else if (l >= 32) src = 31;
                if (src >= 0 && !f[l]) failed |= !seq_scan_step(nn[l], ff[l], ss[l], n[src], f[src], st[src]);
            }
            for (int l = 0; l < 64; l++) { n[l] = nn[l]; f[l] = ff[l]; st[l] = ss[l]; }
        }
        scan_failed[g] = failed;
        bool uncovered = false;
        for (int l = 0; l < 64; l++) {
            const int b = g * 64 + l;
            const bool pick = ((mask >> l) & 1) && b >= headleaf && b < nleaf && n[l].a != SEQ_ZERO_LEAF;
            const bool valid = (n[l].a >> 24) != 0u;
            if (!pick) continue;
            if (valid) seg[g].push_back(seq_item_of_node(n[l]));
            else if (split_ok[l]) { seg[g].push_back(sp[l].a); seg[g].push_back(sp[l].b); }
            else if (bs[b] <= 3.4028234e38f) for (int i = 0; i < LEAF; i++) seg[g].push_back(seq_item_of_term(p[(size_t)b * LEAF + i]));
            else uncovered = true;
        }
        const bool fits = seg[g].size() <= 128;
        cntw[g] = fits ? (int)seg[g].size() : 0;
        flag[g] = (uncovered ? 1 : 0) | (fits ? 0 : 2);
        for (int l = 0; l < 64; l++) { rec[(size_t)g * 64 + l].a = n[l].a; rec[(size_t)g * 64 + l].b = n[l].b | ((uint32_t)st[l] << 24); }
        items[g] = mask;
    }
    float s = 0.0f;
    for (int k = 0; k < head; k++) s += p[k];
    uint32_t sb = seq_f2u(s);
    uint32_t badm = 0, path = 0; int tot = 0;
    for (int g = 0; g < NH; g++) {
        if (flag[g] || scan_failed[g]) badm |= 1u << g;
        if (flag[g] & 2) path |= RMS_PATH_NOFIT;
        if (flag[g] & 1) { path |= RMS_PATH_UNCOVERED; dbg_reason |= 2; }
        if (scan_failed[g]) { path |= RMS_PATH_SCANFAIL; dbg_reason |= 1; }
        tot += cntw[g];
    }
    if (n_items) *n_items = tot;
    uint32_t why = (badm ? RMS_PATH_FLAGGED : 0u) | (tot > 64 ? RMS_PATH_OVER64 : 0u) | ((uint32_t)(tot & 0xFF) << 8) | ((badm & 0xFFu) << 20);
    if (!badm && tot <= 64) {
        uint32_t t = sb, bad = 0, nsplit = 0, nsingle = 0;
        for (int g = 0; g < NH; g++) for (const SeqItem& it : seg[g]) { t = seq_item_apply(t, it, bad); if (it.e == SEQ_ANY_BINADE) nsingle++; else if (it.x != 0u) nsplit++; }
        if (!bad) { if (path_out) *path_out = ((uint32_t)tot << 16) | (nsplit << 8) | nsingle; return seq_u2f(t); }
        why |= RMS_PATH_CHECK; dbg_reason |= 4;
    }
    // ---- the record walk (rms_walk_fast / rms_walk_heap)
    int replays = 0;
    for (int g = 0; g < NH; g++) {
        int nloc = nleaf - g * 64; nloc = nloc < 0 ? 0 : (nloc > 64 ? 64 : nloc);
        int pos = headleaf - g * 64; pos = pos < 0 ? 0 : pos;
        uint64_t mask = items[g], zm = 0;
        if (pos < 64) mask &= ~0ull << pos; else mask = 0;
        if (nloc < 64) mask &= ~(~0ull << nloc);
        for (int l = 0; l < 64; l++) if (rec[(size_t)g * 64 + l].a == SEQ_ZERO_LEAF) zm |= 1ull << l;
        mask &= ~zm;
        while (mask) {
            const int i = __builtin_ctzll(mask); mask &= mask - 1;
            const uint32_t na = rec[(size_t)g * 64 + i].a, nb = rec[(size_t)g * 64 + i].b;
            const uint32_t e = na >> 24;
            bool ok;
            uint32_t t;
            if (scan_failed[g]) {                                          // rms_walk_heap: the record's start is checked too
                const int st = (int)(nb >> 24);
                if (st > pos && ((((1ull << st) - 1ull) & (~0ull << pos)) & ~zm) == 0ull) pos = st;
                const uint32_t M = (sb & 0x7FFFFFu) | 0x800000u, Mn = M + (((M & 1u) ? nb : na) & 0xFFFFFFu);
                ok = (int)(nb >> 24) == pos && e == (sb >> 23) && e != 0u && Mn < 0x1000000u;
                t = ((sb >> 23) << 23) | (Mn & 0x7FFFFFu);
            } else {
                t = sb + (((sb & 1u) ? nb : na) & 0xFFFFFFu);
                ok = (((t ^ sb) >> 23) | (e ^ (sb >> 23)) | ((e - 1u) >> 31)) == 0u;
            }
            if (ok) sb = t;
            else {
                if (!scan_failed[g]) replays++;
                float f = seq_u2f(sb);
                for (int l = pos; l <= i; l++) { const float* q = p + ((size_t)g * 64 + l) * LEAF; for (int k = 0; k < LEAF; k++) f += q[k]; }
                sb = seq_f2u(f);
            }
            pos = i + 1;
        }
    }
    if (path_out) *path_out = why | path | (uint32_t)(replays > 255 ? 255 : replays);
    return seq_u2f(sb);
}
// *fast = 1 if the list was enough, *n_items = its length
extern "C" float seqsum_items(const float* pin, int K, int NH, int head_terms, int* fast, int* n_items) {
    uint32_t path = 0;
    const float r = seqsum_device(pin, K, NH, head_terms, &path, n_items);
    if (fast) *fast = (path & RMS_PATH_LEFT) ? 0 : 1;
    return r;
}
// the folding-wave counts that ship: rms_nf of the helper counts of the norm-carrying kernels (lnb_seqsum.h); returns how many, at most `cap` written
extern "C" int seqsum_folding_waves(int* out, int cap) {
    const int nh[] = LNB_RMS_NORM_HELPERS;
    int n = 0;
    for (int h : nh) { if (n < cap) out[n] = rms_nf(h); n++; }
    return n;
}
