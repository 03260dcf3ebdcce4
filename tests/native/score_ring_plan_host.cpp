// Host harness of the ring form in moc_amd/csrc/moc_scores_plan.h for tests/test_score_ring_plan_cpu.py: for every point of
// a grid of shapes and request bits it prints the plan with the ring bit and without it, and checks RingLds (regions in
// order, aligned, inside the launch) where the ring form is chosen.
#include <cstdio>
#include <initializer_list>

#include "moc_scores_plan.h"

static int bad = 0;
static void fail(const char* what, int D, int n) {
    if (++bad <= 20) fprintf(stderr, "D=%d n=%d: %s\n", D, n, what);
}

int main() {
    printf("const max_lds=%zu beside=%zu slot=%zu min=%d max=%d form_ring=%d err_ring_ticket=%d\n", SCORE_MAX_LDS, SCORE_RING_BESIDE_LDS,
           SCORE_RING_SLOT, SCORE_RING_SLOTS_MIN, SCORE_RING_SLOTS_MAX, (int)SCORE_RING, (int)SCORE_PLAN_RING_TICKET);
    const int Ds[] = {256, 512, 768, 1024};
    const int dtypes[] = {MOC_F32, MOC_BF16, MOC_F16};
    const int Ces[] = {6, 7, 16, 17, 64};
    const long slides[][3] = {{1, 40, 40}, {6, 382, 300}, {32, 240000, 9000}, {202, 1800000, 60000}, {1100, 2200, 3}};
    for (int D : Ds) for (int dt : dtypes) for (int Ce : Ces) for (auto& s : slides) for (int ticket : {0, 1}) for (int reserved : {0, 1}) {
        ScoreShape q = {D, dt, bank_nt(Ce), (int)s[0], s[1], (int)s[2], ticket != 0, reserved != 0, 0, false};
        const ScorePlan P0 = score_plan(q);
        q.ring = true;
        const ScorePlan P1 = score_plan(q);
        printf("plan %d %d %d %ld %ld %d %d | form=%d unit=%d smem=%zu gx=%d ticketed=%d err=%d | form=%d unit=%d smem=%zu gx=%d chunk=%d err=%d\n", D, dt, Ce,
               s[0], s[1], ticket, reserved, P0.form, P0.unit, P0.smem, P0.gx, (int)P0.ticketed, P0.err, P1.form, P1.unit, P1.smem, P1.gx,
               P1.chunk, P1.err);
        if (!P1.err && P1.form == SCORE_RING) {
            const RingLds L{score_img_bytes(D, dt), (int)s[0], P1.unit};
            const size_t n = (size_t)s[0];
            if (L.ring() != score_img_bytes(D, dt) || L.ring() % 16) fail("ring start", D, (int)n);
            if (L.tiles() != L.ring() + P1.unit * SCORE_RING_SLOT) fail("tiles", D, (int)n);
            if (L.meta() != L.tiles() + 3 * 16 * 17 * 4 || L.meta() % 8) fail("meta", D, (int)n);
            if (L.desc() % 16 || L.desc() < L.meta() + 24 * n + 4 || L.desc() >= L.meta() + 24 * n + 4 + 16) fail("descriptors", D, (int)n);
            if (L.full() != L.desc() + 16 * (size_t)P1.unit || L.free_() != L.full() + 4 * (size_t)P1.unit) fail("flag words", D, (int)n);
            if (L.bytes() != L.free_() + 4 * (size_t)P1.unit || L.bytes() != P1.smem) fail("bytes", D, (int)n);
        }
    }
    printf("bad=%d\n", bad);
    return bad ? 1 : 0;
}
