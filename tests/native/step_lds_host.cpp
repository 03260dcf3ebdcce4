// Host harness of moc_amd/csrc/moc_step_lds.h -- the very header the step kernels carve their dynamic LDS with -- for
// tests/test_step_lds_cpu.py.  Over a grid of shapes it prints the totals the launches ask for (one line per grid point)
// and checks every layout: fields in increasing offset order, no array reaching into the next, the declared alignment,
// the last array's end plus the pad = bytes.  The arrays' extents are written out here a second time, from the field
// comments of the header: that is the point.
#include <cstdio>
#include <string>
#include <vector>

#include "moc_step_lds.h"

using namespace moc_step_lds;

struct Field { const char* name; long off, size; int align; };

static int bad = 0;
static void fail(const char* layout, const std::string& shape, const char* what, const char* field) {
    if (++bad <= 20) fprintf(stderr, "%s %s: %s (%s)\n", layout, shape.c_str(), what, field);
}

// fields in declared order; `pad` and `bytes` of the layout
static void check(const char* layout, const std::string& shape, const std::vector<Field>& f, long pad, long bytes) {
    if (pad < 0) fail(layout, shape, "negative pad", "pad");
    for (size_t i = 0; i < f.size(); ++i) {
        if (f[i].off < 0 || f[i].off % f[i].align) fail(layout, shape, "alignment", f[i].name);
        if (i + 1 < f.size() && f[i].off > f[i + 1].off) fail(layout, shape, "offset order", f[i + 1].name);
        if (i + 1 < f.size() && f[i].off + f[i].size > f[i + 1].off) fail(layout, shape, "overlaps the next array", f[i].name);
    }
    if (f.back().off + f.back().size + pad != bytes) fail(layout, shape, "last end + pad != bytes", f.back().name);
}

static void pool_fields(std::vector<Field>& f, const PoolBlockLds& B, long C, long K, long cap, bool with_list) {
    if (with_list) f.push_back({"list", B.list, C * cap * 8, 8});
    f.push_back({"wmax", B.wmax, C * 16 * 8, 8});
    f.push_back({"pooled_s", B.pooled_s, C * 4, 4});
    f.push_back({"dpool", B.dpool, C * 4, 4});
    f.push_back({"ncand", B.ncand, C * 4, 4});
    f.push_back({"topk_s", B.topk_s, C * K * 4, 4});
    if (B.topk_s + C * K * 4 != B.end) fail("PoolBlockLds", "", "end", "topk_s");
}

int main() {
    const int Cs[] = {1, 2, 3, 7, 8, 9, 13, 15, 16, 17, 30, 37, 61, 64};
    const int Ks[] = {1, 3, 4, 7, 8, 9, 10, 15, 16};
    const int Ds[] = {256, 512, 768, 1024};
    long pool_one_over = 0;
    printf("limits finish=%d pool_step=%d narrow=%d tiles=%d wide=%d\n", FINISH_MAX_LDS, POOL_STEP_MAX_LDS, NARROW_MAX_LDS,
           TILE_MAX_LDS, WIDE_MAX_LDS);
    for (int C : Cs) for (int K : Ks) for (int D : Ds) for (int esz : {2, 4}) for (int train : {0, 1}) {
        const long P = (long)C * K;
        const int cap = step_cap(C);
        char sh[96];
        snprintf(sh, sizeof(sh), "C=%d K=%d D=%d esz=%d train=%d", C, K, D, esz, train);
        const std::string shape = sh;

        const FinishLds F = finish_lds(C, K, train);
        if (train)
            check("FinishLds", shape, {{"dz", F.dz, P * 16, 16}, {"prow", F.prow, P * 4, 4}, {"H1s", F.H1s, (long)FIN_CHUNK * H * 4, 4},
                                       {"W2s", F.W2s, 4 * H * 4, 4}}, F.pad, F.bytes);
        else if (F.bytes != 0) fail("FinishLds", shape, "evaluation takes no dynamic LDS", "bytes");

        const PoolStepLds S = pool_step_lds(C, K, cap, train);
        {
            const long Pt = train ? P : 0;
            std::vector<Field> f;
            pool_fields(f, S.pool, C, K, cap, true);
            f.push_back({"dz", S.dz, Pt * 16, 4});
            f.push_back({"H1s", S.H1s, Pt * H * 4, 4});
            f.push_back({"dhs", S.dhs, Pt * H * 4, 4});
            f.push_back({"W2s", S.W2s, 4 * H * 4, 4});
            check("PoolStepLds", shape, f, S.pad, S.bytes);
            // what step_plan calls pool_one: the launch's bound can never fire for a shape the plan admits
            if (K <= 16 && C <= 16 && (!train || P <= 64) && S.bytes > POOL_STEP_MAX_LDS) ++pool_one_over;
        }

        const NarrowStepLds N = narrow_step_lds(C, K, D, cap);
        {
            std::vector<Field> f;
            pool_fields(f, N.pool, C, K, cap, true);
            f.push_back({"dz", N.dz, P * 16, 4});
            f.push_back({"H1s", N.H1s, P * H * 4, 4});
            f.push_back({"dhs", N.dhs, P * H * 4, 4});
            f.push_back({"W2s", N.W2s, 4 * H * 4, 4});
            f.push_back({"row_s", N.row_s, P * 8, 8});
            f.push_back({"xs", N.xs, P * D * 4, 16});
            check("NarrowStepLds", shape, f, N.pad, N.bytes);
            if (N.pad > NARROW_PAD) fail("NarrowStepLds", shape, "more slack than the named pad", "pad");
        }

        const TileStepLds T = tile_step_lds(C, K, cap);
        {
            if (T.PD != ((P + 3) & ~3L)) fail("TileStepLds", shape, "PD", "dhs");
            std::vector<Field> f = {
                {"plam", T.plam, P * 16, 16}, {"psc", T.psc, P * 16, 16}, {"xs", T.xs, P * 256 * 4, 16}, {"dhs", T.dhs, (long)T.PD * 4, 16},
                {"dz", T.dz, P * 16, 16}, {"list", T.list, (long)C * cap * 8, 8}, {"t0s", T.t0s, C * 8, 8}, {"prid", T.prid, P * 8, 8},
                {"lsrc", T.lsrc, (long)C * TILE_CL * 4, 4}, {"topv", T.topv, C * 16 * 4, 4}, {"pooled_s", T.pooled_s, C * 4, 4},
                {"dpool", T.dpool, C * 4, 4}, {"ncand", T.ncand, C * 4, 4}, {"flagc", T.flagc, C * 4, 4}, {"topk_s", T.topk_s, P * 4, 4},
                {"h1s", T.h1s, P * 4, 4}, {"w2s", T.w2s, 4 * 4, 4}};
            check("TileStepLds", shape, f, T.pad, T.sink);               // the arrays and the pad end where the sink starts
            if (T.sink + TILE_SINK != T.bytes || TILE_SINK != 1024) fail("TileStepLds", shape, "the sink is the last 1,024 bytes", "sink");
            if (T.sink % 4) fail("TileStepLds", shape, "alignment", "sink");
        }

        const int wcap = wide_cap(C), pch = wide_pch(C, K, D, esz);
        const WideStepLds W = wide_step_lds(C, K, D, esz, pch, wcap);
        {
            const long lists = (long)C * wcap * 8, rows = (long)pch * (D / 16) * esz, part = 8 * 4 * 64 * 4;
            if (W.region != 0 || W.region_bytes % 16 || W.region_bytes < ((lists + 15) & ~15L) || W.region_bytes < ((rows + 15) & ~15L))
                fail("WideStepLds", shape, "region holds the lists and a chunk's row pieces, rounded to 16", "region");
            if (W.part != W.region || part > W.region_bytes) fail("WideStepLds", shape, "the partial sums fit in region", "part");
            if (W.pool.list != W.region) fail("WideStepLds", shape, "the lists start the region", "list");
            if (W.PM != ((P + 16 + 3) & ~3L)) fail("WideStepLds", shape, "PM", "mask");
            std::vector<Field> f = {{"region", W.region, W.region_bytes, 16}};
            pool_fields(f, W.pool, C, K, wcap, false);
            f.push_back({"dz", W.dz, (P + 16) * 16, 16});
            f.push_back({"h1o", W.h1o, P * 16, 4});
            f.push_back({"mask", W.mask, 2L * W.PM * 4, 16});
            f.push_back({"sidx_s", W.sidx_s, P * 4, 4});
            f.push_back({"W2s", W.W2s, 4 * H * 4, 4});
            f.push_back({"red", W.red, 32 * 4, 4});
            f.push_back({"prow_s", W.prow_s, P * 8, 8});
            check("WideStepLds", shape, f, W.pad, W.bytes);
            if ((W.PM * 4) % 16) fail("WideStepLds", shape, "the second mask plane is 16-byte aligned too", "mask");
        }
        printf("%d %d %d %d %d finish=%d pool_step=%d narrow=%d tiles=%d sink_off=%d wide=%d wide_region=%d pch=%d wide_cap=%d\n", C, K, D,
               esz, train, F.bytes, S.bytes, N.bytes, T.bytes, T.sink, W.bytes, W.region_bytes, pch, wcap);
    }
    printf("bad=%d pool_one_over=%ld\n", bad, pool_one_over);
    return bad ? 1 : 0;
}
