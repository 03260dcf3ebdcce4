// Hyper-parameter grids: the score pass of one slide shared by the slides that visit the same rows under the same mask
// (include/moc_hip.h moc_stats_share).
//
// Runs that differ only in topj / topk / discard_classifiers train on the same bags and, from equal generator states, draw
// the same masks.  Everything phase A does in front of moc_select -- the kept-row list, the score pass, the row statistics
// -- depends on none of the three, so it runs once for the LEADER slide and this kernel fills the slots of its FOLLOWERS.
// What a later kernel reads per slot of a slide, and therefore what is copied (the whole list: mask_compact_kernel,
// row_epilogue of the score kernels, stats_from_cache_kernel):
//   n_kept[b]                     <- n_kept[l]                          (moc_select, moc_gather_candidates, the next share)
//   kept[row_off[b] + i]          <- kept[row_off[l] + i]               (compact_kernel: sel_row = x_off[b] + kept[...])
//   stats[r][row_off[b] + i]      <- stats[r][row_off[l] + i]           r < 2C+3, or C+5 with MOC_STATS_COMPACT
//   sel_flag[row_off[b] + i]      <- 0                                  (the score pass clears it: the selectors only set)
// for i < n_kept[l].  A copy: no arithmetic touches a value.
#include "moc_common.h"

namespace {

constexpr int SH_THREADS = 256;
constexpr int SH_CHUNK = SH_THREADS * 4;     // 4-byte words of one array row a workgroup copies per round: one uint4 per thread
constexpr int SH_ROWS = 4;                   // array rows in flight per thread (loads of four rows, then their stores; spelled out below)

struct ShareArgs {
    const int32_t* leader_of_slide;
    const int64_t* row_off;
    int32_t* kept;           // nullable (no mask)
    int32_t* n_kept;         // nullable (no mask)
    float* stats;
    uint8_t* sel_flag;
    int64_t stride;          // total_rows
    int n_slides, slide0, NS;
    int vec_ok;              // kept and stats are 16-byte aligned and stride % 4 == 0: a row's alignment follows from row_off alone
};

// grid (row blocks, follower slides), 256 threads
__global__ __launch_bounds__(SH_THREADS) void stats_share_kernel(ShareArgs a) {
    const int b = a.slide0 + (int)blockIdx.y;
    int l = a.leader_of_slide[b];                              // (uniform: one scalar load)
    if (l < 0) return;                                         // not a follower
    l = l < a.n_slides ? l : a.n_slides - 1;                   // clamped into the batch, as model_of_slide is
    if (l == b) return;
    const int64_t src0 = a.row_off[l], dst0 = a.row_off[b];
    const int cap_l = (int)(a.row_off[l + 1] - src0), cap_b = (int)(a.row_off[b + 1] - dst0);
    int nk = a.n_kept ? a.n_kept[l] : cap_l;
    nk = nk < cap_l ? nk : cap_l;                              // never outside either slide's slots
    nk = nk < cap_b ? nk : cap_b;
    nk = nk > 0 ? nk : 0;
    if (blockIdx.x == 0 && threadIdx.x == 0 && a.n_kept) a.n_kept[b] = nk;
    if (nk == 0) return;
    const int t = (int)threadIdx.x;
    // rows of 4-byte words: row 0 the kept list (masked batches), then the NS statistics rows.  Leader and follower share
    // their alignment inside a 16-byte line when their first slots differ by a multiple of four.
    const int first = a.kept ? 0 : 1;
    const bool vec = a.vec_ok && (((src0 - dst0) & 3) == 0);
    const int head = vec ? (int)((4 - (dst0 & 3)) & 3) : 0;    // scalar words in front of the first aligned one
    const int h = head < nk ? head : nk;
    const int nvec = vec ? (nk - h) >> 2 : 0;
    const int tail0 = h + 4 * nvec;                            // scalar words behind the last full vector
    auto row_src = [&](int r) -> const uint32_t* {
        return r == 0 ? reinterpret_cast<const uint32_t*>(a.kept) + src0
                      : reinterpret_cast<const uint32_t*>(a.stats) + (int64_t)(r - 1) * a.stride + src0;
    };
    auto row_dst = [&](int r) -> uint32_t* {
        return r == 0 ? reinterpret_cast<uint32_t*>(a.kept) + dst0
                      : reinterpret_cast<uint32_t*>(a.stats) + (int64_t)(r - 1) * a.stride + dst0;
    };
    const int last = a.NS + 1;                                 // rows [first, last)
    if (vec) {
        for (int v0 = (int)blockIdx.x * SH_THREADS; v0 < nvec; v0 += (int)gridDim.x * SH_THREADS) {
            const int v = v0 + t;
            if (v >= nvec) continue;
            // (named registers, not an array: an indexed private array is moved to LDS by the compiler)
            for (int r0 = first; r0 < last; r0 += SH_ROWS) {
                auto rd = [&](int q) { return reinterpret_cast<const uint4*>(row_src(r0 + q < last ? r0 + q : last - 1) + h)[v]; };
                auto wr = [&](int q, const uint4& p) { if (r0 + q < last) reinterpret_cast<uint4*>(row_dst(r0 + q) + h)[v] = p; };
                const uint4 p0 = rd(0), p1 = rd(1), p2 = rd(2), p3 = rd(3);
                wr(0, p0); wr(1, p1); wr(2, p2); wr(3, p3);
            }
        }
        if (blockIdx.x == 0) {                                 // head and tail: at most three words each per row
            const int n_tail = nk - tail0;
            for (int e = t; e < (last - first) * 8; e += SH_THREADS) {
                const int r = first + (e >> 3), w = e & 7;
                const int i = w < 4 ? w : tail0 + (w - 4);
                const bool ok = w < 4 ? w < h : (w - 4) < n_tail;
                if (ok) row_dst(r)[i] = row_src(r)[i];
            }
        }
    } else {
        for (int i0 = (int)blockIdx.x * SH_CHUNK; i0 < nk; i0 += (int)gridDim.x * SH_CHUNK) {
            for (int r0 = first; r0 < last; r0 += SH_ROWS) {
                auto rd = [&](int q, int u) {
                    const int i = i0 + u * SH_THREADS + t;
                    return row_src(r0 + q < last ? r0 + q : last - 1)[i < nk ? i : nk - 1];
                };
                auto wr = [&](int q, int u, uint32_t w) {
                    const int i = i0 + u * SH_THREADS + t;
                    if (r0 + q < last && i < nk) row_dst(r0 + q)[i] = w;
                };
#define MOC_SH_ROW(q) const uint32_t w##q##0 = rd(q, 0), w##q##1 = rd(q, 1), w##q##2 = rd(q, 2), w##q##3 = rd(q, 3)
                MOC_SH_ROW(0); MOC_SH_ROW(1); MOC_SH_ROW(2); MOC_SH_ROW(3);
#undef MOC_SH_ROW
#define MOC_SH_ROW(q) wr(q, 0, w##q##0); wr(q, 1, w##q##1); wr(q, 2, w##q##2); wr(q, 3, w##q##3)
                MOC_SH_ROW(0); MOC_SH_ROW(1); MOC_SH_ROW(2); MOC_SH_ROW(3);
#undef MOC_SH_ROW
            }
        }
    }
    // the follower's union flags, as the score pass leaves them
    uint8_t* flag = a.sel_flag + dst0;
    for (int i0 = (int)blockIdx.x * SH_CHUNK; i0 < nk; i0 += (int)gridDim.x * SH_CHUNK) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i0 + u * SH_THREADS + t;
            if (i < nk) flag[i] = 0;
        }
    }
}

// The lists-only half of the share (include/moc_hip.h moc_kept_share): a follower whose statistics its OWN score pass
// writes -- a run under another prompt bank, which sees the leader's masks and none of its scores -- needs the leader's
// kept-row list and count and nothing else; the 2C+3 statistics rows and the flags are left to that pass.
struct KeptShareArgs {
    const int32_t* leader_of_slide;
    const int64_t* row_off;
    int32_t* kept;
    int32_t* n_kept;
    int n_slides, slide0;
    int vec_ok;              // kept is 16-byte aligned: a list's alignment follows from row_off alone
};

// grid (row blocks, follower slides), 256 threads
__global__ __launch_bounds__(SH_THREADS) void kept_share_kernel(KeptShareArgs a) {
    const int b = a.slide0 + (int)blockIdx.y;
    int l = a.leader_of_slide[b];                              // (uniform: one scalar load)
    if (l < 0) return;                                         // not a follower
    l = l < a.n_slides ? l : a.n_slides - 1;                   // clamped into the batch, as in stats_share_kernel
    if (l == b) return;
    const int64_t src0 = a.row_off[l], dst0 = a.row_off[b];
    const int cap_l = (int)(a.row_off[l + 1] - src0), cap_b = (int)(a.row_off[b + 1] - dst0);
    int nk = a.n_kept[l];
    nk = nk < cap_l ? nk : cap_l;                              // never outside either slide's slots
    nk = nk < cap_b ? nk : cap_b;
    nk = nk > 0 ? nk : 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) a.n_kept[b] = nk;
    if (nk == 0) return;
    const int t = (int)threadIdx.x;
    const uint32_t* src = reinterpret_cast<const uint32_t*>(a.kept) + src0;
    uint32_t* dst = reinterpret_cast<uint32_t*>(a.kept) + dst0;
    const bool vec = a.vec_ok && (((src0 - dst0) & 3) == 0);
    if (vec) {
        const int head = (int)((4 - (dst0 & 3)) & 3);          // scalar words in front of the first aligned one
        const int h = head < nk ? head : nk;
        const int nvec = (nk - h) >> 2;
        const int tail0 = h + 4 * nvec;                        // scalar words behind the last full vector
        for (int v = (int)blockIdx.x * SH_THREADS + t; v < nvec; v += (int)gridDim.x * SH_THREADS)
            reinterpret_cast<uint4*>(dst + h)[v] = reinterpret_cast<const uint4*>(src + h)[v];
        if (blockIdx.x == 0 && t < 8) {                        // head and tail: at most three words each
            const int i = t < 4 ? t : tail0 + (t - 4);
            const bool ok = t < 4 ? t < h : (t - 4) < nk - tail0;
            if (ok) dst[i] = src[i];
        }
    } else {
        for (int i0 = (int)blockIdx.x * SH_CHUNK; i0 < nk; i0 += (int)gridDim.x * SH_CHUNK) {
            auto rd = [&](int u) { const int i = i0 + u * SH_THREADS + t; return src[i < nk ? i : nk - 1]; };
            auto wr = [&](int u, uint32_t w) { const int i = i0 + u * SH_THREADS + t; if (i < nk) dst[i] = w; };
            const uint32_t w0 = rd(0), w1 = rd(1), w2 = rd(2), w3 = rd(3);
            wr(0, w0); wr(1, w1); wr(2, w2); wr(3, w3);
        }
    }
}

}  // namespace

extern "C" int moc_stats_share(const moc_batch_t* B, const int32_t* leader_of_slide, int slide0, int n, moc_stream_t stream) {
    MOC_REQUIRE(B && leader_of_slide, "moc_stats_share: null pointer");
    if (int rc = moc_check_batch(B, "moc_stats_share")) return rc;
    MOC_REQUIRE(B->stats && B->sel_flag, "moc_stats_share: the batch has no stats / sel_flag");
    MOC_REQUIRE(slide0 >= 0 && n >= 1 && (int64_t)slide0 + n <= B->n_slides, "moc_stats_share: bad slide range [%d, %d + %d) of %d",
                slide0, slide0, n, B->n_slides);
    MOC_REQUIRE(n <= 65535, "moc_stats_share: at most 65535 slides per call, got %d", n);
    ShareArgs a;
    a.leader_of_slide = leader_of_slide;
    a.row_off = B->row_off;
    a.kept = B->mask ? B->kept : nullptr;
    a.n_kept = B->mask ? B->n_kept : nullptr;
    a.stats = B->stats;
    a.sel_flag = B->sel_flag;
    a.stride = B->total_rows;
    a.n_slides = B->n_slides; a.slide0 = slide0;
    a.NS = (B->flags & MOC_STATS_COMPACT) ? B->C + 5 : 2 * B->C + 3;
    a.vec_ok = (((uintptr_t)B->stats & 15) == 0 && (!a.kept || ((uintptr_t)a.kept & 15) == 0) && (B->total_rows & 3) == 0) ? 1 : 0;
    const dim3 grid(moc_cdiv(B->max_rows, SH_CHUNK), n);
    stats_share_kernel<<<grid, SH_THREADS, 0, (hipStream_t)stream>>>(a);
    MOC_CHECK_LAUNCH("moc_stats_share");
    return MOC_OK;
}

extern "C" int moc_kept_share(const moc_batch_t* B, const int32_t* leader_of_slide, int slide0, int n, moc_stream_t stream) {
    MOC_REQUIRE(B && leader_of_slide, "moc_kept_share: null pointer");
    if (int rc = moc_check_batch(B, "moc_kept_share")) return rc;
    MOC_REQUIRE(slide0 >= 0 && n >= 1 && (int64_t)slide0 + n <= B->n_slides, "moc_kept_share: bad slide range [%d, %d + %d) of %d",
                slide0, slide0, n, B->n_slides);
    MOC_REQUIRE(n <= 65535, "moc_kept_share: at most 65535 slides per call, got %d", n);
    if (!B->mask) return MOC_OK;                               // no lists: every slide keeps all of its rows
    MOC_REQUIRE(B->kept && B->n_kept, "moc_kept_share: a masked batch without kept / n_kept");
    KeptShareArgs a;
    a.leader_of_slide = leader_of_slide;
    a.row_off = B->row_off;
    a.kept = B->kept;
    a.n_kept = B->n_kept;
    a.n_slides = B->n_slides; a.slide0 = slide0;
    a.vec_ok = ((uintptr_t)B->kept & 15) == 0 ? 1 : 0;
    const dim3 grid(moc_cdiv(B->max_rows, SH_CHUNK), n);
    kept_share_kernel<<<grid, SH_THREADS, 0, (hipStream_t)stream>>>(a);
    MOC_CHECK_LAUNCH("moc_kept_share");
    return MOC_OK;
}
