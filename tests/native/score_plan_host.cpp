// Host harness of moc_amd/csrc/moc_scores_plan.h -- the very header moc_scores and moc_scores_banks plan their launches
// with -- for tests/test_score_plan_cpu.py.  It prints score_plan over the grid of tests/golden/make_score_plan.py (one line
// per point: the moc_scores grid, then the moc_scores_banks grid, then the extras) and, for every streaming point, checks
// StreamLds against the layout the kernels carve by hand: regions in order, disjoint, aligned (16 B images, 8 B
// metadata), bytes(chunk) within the limit, the ticketed walk's s_counter word behind the chunk's metadata and inside the
// launch.  The regions' extents are written out here a second time, from the kernels' carve: that is the point.
#include <cstdio>
#include <initializer_list>

#include "moc_scores_plan.h"

static int bad = 0;
static void fail(const char* shape, const char* what) {
    if (++bad <= 20) fprintf(stderr, "%s: %s\n", shape, what);
}

static void check_stream(const char* shape, const ScoreShape& q, const ScorePlan& P) {
    const StreamLds L{score_img_bytes(q.D, q.dtype), q.NT};
    const long n = P.chunk, NT = q.NT;
    const long img = q.dtype != MOC_F32 ? (q.D / 32) * 3 * 1024 : (q.D / 16) * 1024;
    // {offset, size, alignment} as scores_stream_kernel / scores_banks_kernel carve a launch over n slides
    const long reg[][3] = {{(long)L.images(), NT * img, 16},          {(long)L.tiles(), 4 * 16 * (NT * 16 + 1) * 4, 4},
                           {(long)L.first_slot(n), 8 * n, 8},         {(long)L.first_row(n), 8 * n, 8},
                           {(long)L.prefix(n), 4 * (n + 1), 4},       {(long)L.kept_rows(n), 4 * n, 4},
                           {(long)L.meta_end(n), 0, 4}};
    if (reg[0][0] != 0) fail(shape, "the images start the launch's LDS");
    for (int i = 0; i < 7; ++i) {
        if (reg[i][0] % reg[i][2]) fail(shape, "alignment");
        if (i + 1 < 7 && reg[i][0] + reg[i][1] != reg[i + 1][0]) fail(shape, "a region does not end where the next starts");
    }
    if ((long)L.meta() != NT * img + 4 * 16 * (NT * 16 + 1) * 4) fail(shape, "meta()");
    if ((long)L.fixed() != (long)L.meta() + 16 || L.bytes(P.chunk) != L.fixed() + 24 * (size_t)n) fail(shape, "fixed() / bytes()");
    if (P.smem != L.bytes(P.chunk) || P.smem > SCORE_MAX_LDS) fail(shape, "bytes(chunk) within 160 KiB, and what the plan launches with");
    if (P.chunk < 1 || P.chunk > L.chunk_max() || L.bytes(L.chunk_max() + 1) <= SCORE_MAX_LDS) fail(shape, "chunk_max()");
    // (int*)meta + 6 n + 1, one word
    if ((long)L.counter(n) != (long)L.meta() + 4 * (6 * n + 1)) fail(shape, "s_counter is not where the kernel writes it");
    if (L.counter(n) < L.meta_end(n) || L.counter(n) + 4 > L.bytes(P.chunk)) fail(shape, "s_counter outside [meta end, bytes(chunk))");
}

static void line(const char* shape, const ScoreShape& q) {
    const ScorePlan P = score_plan(q);
    if (P.err)
        printf("%s form=%d unit=0 NT=%d ticketed=0 smem=0 chunk=0 gx=0 gy=0 tpw=0 err=%d need=%zu\n", shape, P.form, P.NT, P.err, P.need);
    else
        printf("%s form=%d unit=%d NT=%d ticketed=%d smem=%zu chunk=%d gx=%d gy=%d tpw=%d err=0 need=0\n", shape, P.form, P.unit, P.NT,
               (int)P.ticketed, P.smem, P.chunk, P.gx, P.gy, P.tpw);
    if (!P.err && P.form == SCORE_STREAM) check_stream(shape, q, P);
}

int main() {
    const int Ds[] = {256, 512, 768, 1024, 1280, 2048};
    const int dtypes[] = {MOC_F32, MOC_BF16, MOC_F16};
    const int Ces[] = {3, 16, 17, 32, 33, 48, 49, 64, 65, 80, 81, 96, 128, 129, 256};
    const long slides[][3] = {{1, 1, 1}, {32, 9000, 900}, {202, 1800000, 60000}, {1100, 2200, 3}, {3000, 6000, 4}};
    char sh[128];
    for (int D : Ds) for (int dt : dtypes) for (int Ce : Ces) for (auto& s : slides) for (int ticket : {0, 1}) {
        snprintf(sh, sizeof(sh), "scores %d %d %d %ld %ld %ld %d", D, dt, Ce, s[0], s[1], s[2], ticket);
        line(sh, {D, dt, bank_nt(Ce), (int)s[0], s[1], (int)s[2], ticket != 0, false, 0, false});
    }
    for (int D : Ds) for (int dt : dtypes) for (int G : {1, 2, 3, 4}) for (auto& s : slides) {
        snprintf(sh, sizeof(sh), "banks %d %d %d %ld %ld %ld", D, dt, G, s[0], s[1], s[2]);
        line(sh, {D, dt, G, (int)s[0], s[1], (int)s[2], false, false, 0, true});
    }
    // D, dtype, Ce, slides, ticket, look-ahead cap, reserved set
    const long extras[][9] = {{512, MOC_F32, 3, 202, 1800000, 60000, 1, 96, 0}, {512, MOC_F32, 3, 202, 1800000, 60000, 0, 96, 0},
                              {512, MOC_BF16, 33, 32, 9000, 900, 1, 64, 1},     {256, MOC_F32, 64, 32, 9000, 900, 1, 64, 1},
                              {512, MOC_F32, 3, 1, 1, 1, 1, 96, 0},             {512, MOC_BF16, 3, 32, 9000, 900, 0, 0, 1},
                              {256, MOC_BF16, 49, 32, 9000, 900, 0, 0, 1}};
    for (auto& e : extras) {
        snprintf(sh, sizeof(sh), "extra %ld %ld %ld %ld %ld %ld %ld %ld %ld", e[0], e[1], e[2], e[3], e[4], e[5], e[6], e[7], e[8]);
        line(sh, {(int)e[0], (int)e[1], bank_nt((int)e[2]), (int)e[3], e[4], (int)e[5], e[6] != 0, e[8] != 0, (int)e[7], false});
    }
    // the one-liners of the library's size queries
    for (int D : {256, 512, 1024}) printf("banks_max %d %d %d %d\n", D, score_banks_max(D, MOC_F32), score_banks_max(D, MOC_BF16), score_banks_max(D, MOC_F16));
    printf("bad=%d\n", bad);
    return bad ? 1 : 0;
}
