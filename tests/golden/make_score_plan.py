#!/usr/bin/env python3
"""Write tests/golden/score_plan.json: what the score pass launches -- kernel form, NF / CH, n-tiles, ticketed or not,
dynamic LDS, slides per chunk, grid, tpw, or the refusal -- over a grid of shapes, from the host code of scores_impl
(moc_scores.hip) and moc_scores_banks (moc_scores_banks.hip) at commit 9e114ba ("Nystrom layer: landmark pseudo-inverse as
a chain of HIP products"): the last commit in which the two entries sized and chose their launches each with formulas of
its own, transcribed below as integer arithmetic.  score_plan of moc_amd/csrc/moc_scores_plan.h must give the same
(tests/test_score_plan_cpu.py): the bytes of a launch decide how many workgroups share a CU, and the form which kernel
runs.

    python -B tests/golden/make_score_plan.py

checks the recorder against anchors worked out by hand and rewrites the file."""
import itertools
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
RECORD = os.path.join(HERE, "score_plan.json")
PARENT = "9e114ba"

F32, BF16, F16 = 0, 1, 2                       # MOC_F32, MOC_BF16, MOC_F16
AXES = {
    "D": [256, 512, 768, 1024, 1280, 2048],
    "dtype": [F32, BF16, F16],
    "Ce": [3, 16, 17, 32, 33, 48, 49, 64, 65, 80, 81, 96, 128, 129, 256],
    "slides": [[1, 1, 1], [32, 9000, 900], [202, 1800000, 60000], [1100, 2200, 3], [3000, 6000, 4]],   # n_slides, total_rows, max_rows
    "ticket": [0, 1],
}
BANK_AXES = {"D": AXES["D"], "dtype": AXES["dtype"], "G": [1, 2, 3, 4], "slides": AXES["slides"]}
# beside the grid: the look-ahead cap (last but one) and a reserved set (last) -- D, dtype, Ce, slides, ticket, cap, reserved
EXTRAS = [[512, F32, 3, [202, 1800000, 60000], 1, 96, 0], [512, F32, 3, [202, 1800000, 60000], 0, 96, 0],
          [512, BF16, 33, [32, 9000, 900], 1, 64, 1], [256, F32, 64, [32, 9000, 900], 1, 64, 1],
          [512, F32, 3, [1, 1, 1], 1, 96, 0], [512, BF16, 3, [32, 9000, 900], 0, 0, 1], [256, BF16, 49, [32, 9000, 900], 0, 0, 1]]
FORMS = ["stream", "wide_ring", "wide", "generic"]
ERRS = ["ok", "slides_lds", "reserved", "row_lds", "no_stream"]
FIELDS = ["form", "unit", "NT", "ticketed", "smem", "chunk", "gx", "gy", "tpw", "err", "need"]

LDS = 160 * 1024
WD_R = 4


def cdiv(a, b):
    return (a + b - 1) // b


def img_bytes(D, dtype):
    return (D // 32) * 3 * 1024 if dtype != F32 else (D // 16) * 1024


def tile_bytes(NT):
    return 4 * 16 * (NT * 16 + 1) * 4


def refusal(form, NT, err, need):
    return [FORMS.index(form), 0, NT, 0, 0, 0, 0, 0, 0, ERRS.index(err), need]


def stream_launch(D, dtype, NT, fixed, n_slides, total_rows):
    chunk_max = (LDS - fixed) // 24
    chunk = min(n_slides, chunk_max)
    smem = fixed + chunk * 24
    tiles = (total_rows + 15) // 16 + 2 * n_slides
    wgs = min((tiles + 3) // 4, 256 * (2 if smem <= 80 * 1024 else 1))
    row_b = D * (4 if dtype == F32 else 2)
    return chunk, smem, wgs, 16 if row_b % 1024 == 0 else 8


def scores(D, dtype, Ce, slides, ticket, cap=0, reserved=0):
    """scores_impl"""
    n_slides, total_rows, max_rows = slides
    bf = dtype != F32
    NT = (Ce + 15) // 16
    img = img_bytes(D, dtype)
    fixed = NT * img + tile_bytes(NT) + 16
    if NT <= (3 if bf else 4) and fixed + 24 <= LDS:
        chunk, smem, wgs, nf = stream_launch(D, dtype, NT, fixed, n_slides, total_rows)
        if not (NT > 1 or chunk == n_slides):
            return refusal("stream", NT, "slides_lds", fixed + n_slides * 24)
        if ticket and cap > 0:
            wgs = min(wgs, cap)
        if reserved and not ticket:
            return refusal("stream", NT, "reserved", 0)
        return [FORMS.index("stream"), nf, NT, int(bool(ticket) and NT != 4), smem, chunk, wgs, 1, 0, 0, 0]
    if bf and 4 <= NT <= 8 and D % 64 == 0:
        kc = 1 if NT <= 6 else 2
        buf = NT * kc * 3 * 1024 + 4 * WD_R * kc * 1024
        smem_w = max(2 * buf, tile_bytes(NT))
        gx = cdiv(max_rows, 4 * WD_R * 16)
        if NT <= 5:
            ring = 3 * (((NT * 3 + 3) // 4) * 4 * 1024)
            return [FORMS.index("wide_ring"), 0, NT, 0, max(ring, tile_bytes(NT)), n_slides, gx, n_slides, 0, 0, 0]
        if smem_w < LDS:
            return [FORMS.index("wide"), 0, NT, 0, smem_w, n_slides, gx, n_slides, 0, 0, 0]
    smem = img + tile_bytes(NT)
    if smem > LDS:
        return refusal("generic", NT, "row_lds", smem)
    return [FORMS.index("generic"), 512 if D % 512 == 0 else 256, NT, 0, smem, n_slides, cdiv(max_rows, 64), n_slides, 1, 0, 0]


def banks_fixed_lds(D, G, dtype):
    return G * img_bytes(D, dtype) + tile_bytes(G) + 16


def banks_max(D, dtype):
    """moc_scores_banks_max"""
    if D <= 0 or D % 256 or dtype not in (F32, BF16, F16):
        return 0
    g = 3 if dtype != F32 else 4
    while g > 0 and banks_fixed_lds(D, g, dtype) + 24 > LDS:
        g -= 1
    return g


def bank_bytes(D, Ce, dtype):
    """moc_bank_bytes"""
    return 0 if D <= 0 or Ce <= 0 else img_bytes(D, dtype) * ((Ce + 15) // 16)


def bank_set_bytes(D, n_banks, dtype):
    """moc_bank_set_bytes"""
    return 0 if D <= 0 or n_banks <= 0 else n_banks * img_bytes(D, dtype)


def banks(D, dtype, G, slides):
    """moc_scores_banks: refused (before any sizing) where G exceeds moc_scores_banks_max"""
    n_slides, total_rows, _ = slides
    if G > banks_max(D, dtype):
        return refusal("stream", G, "no_stream", banks_fixed_lds(D, 1, dtype) + 24)
    chunk, smem, wgs, nf = stream_launch(D, dtype, G, banks_fixed_lds(D, G, dtype), n_slides, total_rows)
    return [FORMS.index("stream"), nf, G, 0, smem, chunk, wgs, 1, 0, 0, 0]


def check_anchors():
    f = dict(zip(FIELDS, range(len(FIELDS))))
    big = [202, 1800000, 60000]
    # bf16, D = 512, one n-tile, 202 slides
    assert img_bytes(512, BF16) == 49152 and 49152 + 4352 + 16 == 53520
    r = scores(512, BF16, 16, big, 0)
    assert r[f["smem"]] == 53520 + 202 * 24 == 58368 <= 80 * 1024 and r[f["gx"]] == 512 and r[f["chunk"]] == 202
    # bf16, D = 1024, one n-tile: fixed 102,672 B, 2,548 slides a launch.  moc_scores refuses a one-n-tile batch that
    # would need chunks (NT > 1 || chunk == n_slides); moc_scores_banks sends it out in two
    assert banks_fixed_lds(1024, 1, BF16) == 102672 and (LDS - 102672) // 24 == 2548
    r = banks(1024, BF16, 1, [3000, 6000, 4])
    assert r[f["chunk"]] == 2548 and cdiv(3000, r[f["chunk"]]) == 2 and r[f["smem"]] == 102672 + 2548 * 24
    assert scores(1024, BF16, 16, [3000, 6000, 4], 0) == refusal("stream", 1, "slides_lds", 102672 + 3000 * 24)
    # fp32, D = 1024, two n-tiles
    assert 2 * img_bytes(1024, F32) == 131072 and 131072 + 8448 + 16 == 139536 and (LDS - 139536) // 24 == 1012
    r = scores(1024, F32, 32, [1100, 2200, 3], 0)
    assert r[f["form"]] == 0 and r[f["chunk"]] == 1012 and cdiv(1100, 1012) == 2 and r[f["smem"]] == 139536 + 1012 * 24
    # the table tests/test_gpu_banks.py asserts
    assert [(banks_max(D, F32), banks_max(D, BF16), banks_max(D, F16)) for D in (256, 512, 1024)] == [(4, 3, 3), (4, 3, 3), (2, 1, 1)]
    # four n-tiles (fp32) drop the ticket; the look-ahead cap needs one
    assert scores(256, F32, 64, big, 1)[f["ticketed"]] == 0 and scores(256, F32, 48, big, 1)[f["ticketed"]] == 1
    assert scores(512, F32, 3, big, 1, 96)[f["gx"]] == 96 and scores(512, F32, 3, big, 0, 96)[f["gx"]] == 512
    # the forms' thresholds: bf16 leaves the streaming form at four n-tiles, the ring at six, wide at eight (two chunk
    # buffers of 8 x 6 + 32 KiB are the whole 160 KiB, and the bound is strict)
    assert [FORMS[scores(256, BF16, Ce, big, 0)[0]] for Ce in (48, 49, 80, 81, 112, 113)] == \
        ["stream", "wide_ring", "wide_ring", "wide", "wide", "generic"]
    assert FORMS[scores(256, F32, 65, big, 0)[0]] == "generic"
    assert scores(2048, BF16, 3, big, 0) == refusal("generic", 1, "row_lds", 64 * 3 * 1024 + 4352)


def record():
    return {"parent": PARENT, "axes": AXES, "bank_axes": BANK_AXES, "extras": EXTRAS, "forms": FORMS, "errs": ERRS, "fields": FIELDS,
            "rows": [scores(*pt) for pt in itertools.product(*AXES.values())],
            "bank_rows": [banks(*pt) for pt in itertools.product(*BANK_AXES.values())],
            "extra_rows": [scores(*pt) for pt in EXTRAS]}


if __name__ == "__main__":
    check_anchors()
    with open(RECORD, "w") as f:
        json.dump(record(), f, separators=(",", ":"))
        f.write("\n")
    print("wrote", RECORD)
