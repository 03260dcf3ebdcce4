// Sensitivity sweeps: the top-K mean at SEVERAL K from ONE ranking (include/moc_hip.h moc_topk_mean_multi).
//
// moc_topk_mean sums the pooled values sequentially in rank order for K <= 64 (moc_select.hip: topk_mean_kernel's
// `k <= 64` branch, topk_mean_wave_kernel), so the K-th prefix of the ranking to Kmax is bit for bit what a launch at that
// K alone gives.  One wave per (segment, class) task, WS_WAVES tasks per workgroup, no workgroup barrier -- the
// arrangement of topk_mean_wave_kernel, which stops at K <= 16; this one goes to 64 (one rank per lane).
#include "moc_common.h"

namespace {

constexpr int WS_CAP = 1024;         // candidate entries per wave (8 KB of LDS; sixteen per lane in registers)
constexpr int WS_SLOTS = WS_CAP / 64;
constexpr int WS_WAVES = 4;          // tasks per workgroup
constexpr int WS_MAX_K = 64;         // one rank per lane; above it the existing kernels sum in a pairwise tree
constexpr int WS_MAX_NK = 8;

struct TopkMultiArgs {
    const float* keys;
    const float* vals;
    const int64_t* seg_off;
    const int32_t* seg_len;   // nullable
    float* pooled;            // [n_K, n_seg, C]
    int32_t* idx_out;         // nullable [n_seg, C, Kmax]
    int32_t* cnt_out;         // nullable [n_seg, C]
    int64_t key_stride, val_stride;
    int C, n_seg, smallest, n_K, Kmax;
    int Ks[WS_MAX_NK];        // by value: no load between the ranking and the stores
};

__global__ __launch_bounds__(64 * WS_WAVES) void topk_mean_multi_kernel(TopkMultiArgs a, int n_tasks) {
    __shared__ unsigned long long cand_s[WS_WAVES][WS_CAP];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int task = blockIdx.x * WS_WAVES + wave;
    if (task >= n_tasks) return;                                   // (no barrier below: waves are on their own)
    const int seg = task / a.C, c = task - seg * a.C;
    const int64_t base = a.seg_off[seg];
    const int n = a.seg_len ? a.seg_len[seg] : (int)(a.seg_off[seg + 1] - base);
    const int out = seg * a.C + c;
    const int64_t slab = (int64_t)a.n_seg * a.C;
    if (n <= 0) {   // mean over an empty set: NaN, like torch -- for every K
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < WS_MAX_NK; ++i)
                if (i < a.n_K) a.pooled[i * slab + out] = __uint_as_float(0x7FC00000u);
            if (a.cnt_out) a.cnt_out[out] = 0;
        }
        if (a.idx_out && lane < a.Kmax) a.idx_out[(int64_t)out * a.Kmax + lane] = -1;
        return;
    }
    const float* kcol = a.keys + (int64_t)c * a.key_stride + base;
    const float* vcol = a.vals + (int64_t)c * a.val_stride + base;
    const uint32_t flip = a.smallest ? 0xFFFFFFFFu : 0u;
    // (clamped, not branched: the loads of a batch go out together; a slot past the segment reads its last key and is
    // masked to zero, below every real entry)
    auto key_at = [&](int i) -> uint32_t {
        const uint32_t uk = moc_key_desc(kcol[i < n ? i : n - 1]) ^ flip;
        return i < n ? uk : 0u;
    };
    const int k = a.Kmax < n ? a.Kmax : n;
    unsigned long long* cand = cand_s[wave];
    unsigned long long mine[WS_SLOTS];
#pragma unroll
    for (int q = 0; q < WS_SLOTS; ++q) mine[q] = 0ull;
    bool listed = false;                                           // wave-uniform: `mine` holds every candidate
    int n_listed = 0;
    if (n <= WS_CAP) {
        // short segments (the mixed scores of a slide's selected rows): every key is a candidate
#pragma unroll
        for (int q = 0; q < WS_SLOTS; ++q) {
            if (q * 64 >= n) break;                                // (uniform)
            const int i = q * 64 + lane;
            const uint32_t u = key_at(i);
            mine[q] = i < n ? ((unsigned long long)u << 32) | (uint32_t)(~(uint32_t)i) : 0ull;
        }
        listed = true;
        n_listed = n;
    } else {
        // ---- the bound: the k-th largest of the TWO largest keys of every lane (128 keys of distinct rows, so k <= 64 of
        // them are >= it: a lower bound of the k-th largest key) over (a) eight runs of 256 consecutive keys spread over the
        // segment -- long segments: the kernel is bound by the bytes of its passes over the keys -- or (b) all keys.  Two
        // per lane, not the lane maximum alone: at k = 64 the smallest of 64 lane maxima of 32 sampled keys each lets an
        // eighth of a segment through.  (n > 1024: every lane holds two keys.)
        auto lane_bound = [&](bool sample) -> uint32_t {
            uint32_t m1 = 0, m2 = 0;
            auto offer = [&](uint32_t u) {
                const uint32_t lo = u < m1 ? u : m1;
                m1 = u > m1 ? u : m1;
                m2 = lo > m2 ? lo : m2;
            };
            if (sample) {
                for (int r = 0; r < 8; ++r) {
                    const int start = (int)(((int64_t)r * n) >> 3);
                    uint32_t u[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) u[q] = key_at(start + q * 64 + lane);
#pragma unroll
                    for (int q = 0; q < 4; ++q) offer(u[q]);
                }
            } else {
                for (int i0 = 0; i0 < n; i0 += 512) {
                    uint32_t u[8];
#pragma unroll
                    for (int q = 0; q < 8; ++q) u[q] = key_at(i0 + q * 64 + lane);
#pragma unroll
                    for (int q = 0; q < 8; ++q) offer(u[q]);
                }
            }
            uint32_t T = 0;
            for (int r = 0; r < k; ++r) {                           // k rounds, one key knocked out per round
                const uint32_t best = (uint32_t)wave_max_u64((unsigned long long)m1);
                const unsigned long long m = __ballot(m1 == best);
                const int first = __ffsll((long long)m) - 1;
                if (lane == first) { m1 = m2; m2 = 0u; }
                T = best;
            }
            return T;
        };
        // ---- the sweep: candidates >= T0, positions by ballot prefix
        auto collect = [&](uint32_t T0) -> int {
            int cnt = 0;
            for (int i0 = 0; i0 < n; i0 += 512) {
                uint32_t u[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) u[q] = key_at(i0 + q * 64 + lane);
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const int i = i0 + q * 64 + lane;
                    const bool hit = i < n && u[q] >= T0;
                    const unsigned long long m = __ballot(hit);
                    if (m == 0ull) continue;                        // (uniform)
                    const int pos = cnt + __popcll(m & ((1ull << lane) - 1ull));
                    if (hit && pos < WS_CAP) cand[pos] = ((unsigned long long)u[q] << 32) | (uint32_t)(~(uint32_t)i);
                    cnt += __popcll(m);
                }
            }
            return cnt;
        };
        const bool sampled = n > 4096;
        int cnt = collect(lane_bound(sampled));
        if (cnt > WS_CAP && sampled) cnt = collect(lane_bound(false));   // (the runs were not typical of the segment: the bound from all keys)
        if (cnt <= WS_CAP) {
            __builtin_amdgcn_wave_barrier();
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // the wave's own LDS writes, before it reads them back
#pragma unroll
            for (int q = 0; q < WS_SLOTS; ++q) {
                if (q * 64 >= cnt) break;                           // (uniform)
                mine[q] = q * 64 + lane < cnt ? cand[q * 64 + lane] : 0ull;
            }
            listed = true;
            n_listed = cnt;
        }
    }
    // ---- the k largest in order; lane r keeps entry r (k <= 64)
    unsigned long long mylist = 0ull;
    if (listed) {
        const int nq = (n_listed + 63) >> 6;                        // slots in use (uniform)
        for (int r = 0; r < k; ++r) {
            unsigned long long best = 0ull;
#pragma unroll
            for (int q = 0; q < WS_SLOTS; ++q)
                if (q < nq) best = mine[q] > best ? mine[q] : best;
            best = wave_max_u64(best);                              // entries are distinct (row in the low word)
#pragma unroll
            for (int q = 0; q < WS_SLOTS; ++q)
                if (q < nq) mine[q] = mine[q] == best ? 0ull : mine[q];
            if (lane == r) mylist = best;
        }
    } else {
        // the list overflowed even with the bound from all keys (flat key distributions): k rounds over ALL keys, each
        // finding the largest entry below the previous one (slow, exact, rare)
        unsigned long long prev = 0ull;
        for (int r = 0; r < k; ++r) {
            unsigned long long best = 0ull;
            for (int i0 = 0; i0 < n; i0 += 256) {
                uint32_t u[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) u[q] = key_at(i0 + q * 64 + lane);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int i = i0 + q * 64 + lane;
                    const unsigned long long e = i < n ? ((unsigned long long)u[q] << 32) | (uint32_t)(~(uint32_t)i) : 0ull;
                    best = ((r == 0 || e < prev) && e > best) ? e : best;
                }
            }
            best = wave_max_u64(best);
            if (lane == r) mylist = best;
            prev = best;
        }
    }
    if (a.idx_out && lane < a.Kmax)
        a.idx_out[(int64_t)out * a.Kmax + lane] = lane < k ? (int32_t)(~(uint32_t)(mylist & 0xFFFFFFFFull)) : -1;
    // the value of rank `lane`: the key read backwards where keys and values are one array (a canonical zero does not say
    // which zero it was), gathered otherwise -- as moc_topk_mean takes it
    const bool same = a.keys == a.vals && a.key_stride == a.val_stride;
    float v = 0.f;
    if (lane < k) {
        const uint32_t u = (uint32_t)(mylist >> 32) ^ flip;
        if (same && u != 0x80000000u) v = __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u);
        else v = vcol[(int)(~(uint32_t)(mylist & 0xFFFFFFFFull))];
    }
    // one running sum over the ranks; at every r + 1 that is some K's min(K, len), that K's mean
    float sum = 0.f;
    for (int r = 0; r < k; ++r) {
        sum += __shfl(v, r, 64);
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < WS_MAX_NK; ++i)
                if (i < a.n_K && (a.Ks[i] < n ? a.Ks[i] : n) == r + 1) a.pooled[i * slab + out] = sum / (float)(r + 1);
        }
    }
    if (lane == 0 && a.cnt_out) a.cnt_out[out] = k;
}

}  // namespace

extern "C" int moc_topk_mean_multi(const float* keys, int64_t key_stride, const float* vals, int64_t val_stride,
                                   const int64_t* seg_off, const int32_t* seg_len, int n_seg, int C,
                                   const int32_t* Ks, int n_K, int smallest, float* pooled, int32_t* idx_out,
                                   int32_t* cnt_out, moc_stream_t stream) {
    MOC_REQUIRE(keys && vals && seg_off && pooled && Ks, "moc_topk_mean_multi: null pointer");
    MOC_REQUIRE(n_seg >= 1 && C >= 1 && (int64_t)n_seg * C <= 0x7FFFFFFF / WS_MAX_K, "moc_topk_mean_multi: bad n_seg=%d C=%d", n_seg, C);
    MOC_REQUIRE(n_K >= 1 && n_K <= WS_MAX_NK, "moc_topk_mean_multi: n_K=%d outside [1, %d]", n_K, WS_MAX_NK);
    TopkMultiArgs a = {};
    a.keys = keys; a.vals = vals; a.seg_off = seg_off; a.seg_len = seg_len; a.pooled = pooled;
    a.idx_out = idx_out; a.cnt_out = cnt_out; a.key_stride = key_stride; a.val_stride = val_stride;
    a.C = C; a.n_seg = n_seg; a.smallest = smallest ? 1 : 0; a.n_K = n_K;
    for (int i = 0; i < n_K; ++i) {
        MOC_REQUIRE(Ks[i] >= 1 && Ks[i] <= WS_MAX_K, "moc_topk_mean_multi: K=%d outside [1, %d]", Ks[i], WS_MAX_K);
        a.Ks[i] = Ks[i];
        a.Kmax = Ks[i] > a.Kmax ? Ks[i] : a.Kmax;
    }
    const int n_tasks = n_seg * C;
    topk_mean_multi_kernel<<<moc_cdiv(n_tasks, WS_WAVES), 64 * WS_WAVES, 0, (hipStream_t)stream>>>(a, n_tasks);
    MOC_CHECK_LAUNCH("moc_topk_mean_multi");
    return MOC_OK;
}
