#!/usr/bin/env python3
"""Write tests/golden/step_lds.json: the dynamic LDS every step kernel's launch asks for, over a grid of shapes, from the
host formulas of moc_meta.hip at commit e2bda5c ("Step kernel: class wave ends at the winners, means on the fourth wave")
-- the last commit in which the host sized the launches with formulas of its own (fused_step_smem, tiles_step_smem,
wide_region, wide_smem, wide_cap, wide_pch and the two formulas inline in launch_finish / launch_pool_finish), transcribed
below as integer arithmetic.  The layouts of moc_amd/csrc/moc_step_lds.h must give the same numbers
(tests/test_step_lds_cpu.py): the bytes of a launch decide how many workgroups share a CU and which kernel a shape gets.

    python -B tests/golden/make_step_lds.py

checks the recorder against anchors worked out by hand and rewrites the file."""
import itertools
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
RECORD = os.path.join(HERE, "step_lds.json")
PARENT = "e2bda5c"

AXES = {
    "C": [1, 2, 3, 7, 8, 9, 13, 15, 16, 17, 30, 37, 61, 64],
    "K": [1, 3, 4, 7, 8, 9, 10, 15, 16],
    "D": [256, 512, 768, 1024],
    "esz": [2, 4],
    "train": [0, 1],
}
FIELDS = ["finish", "pool_step", "narrow", "tiles", "sink_off", "wide", "wide_region", "pch", "wide_cap"]

H = 64
FIN_CHUNK = 256
PS_CAP_MAX = 1024
FS_MAX_DYN_LDS = 160 * 1024 - 64
TILES_SINK = 1024
WD_PCH_MIN = 128


def step_cap(C):
    return PS_CAP_MAX if C <= 8 else PS_CAP_MAX // 2


def finish_smem(C, K, train):                      # launch_finish
    return C * K * (4 * 4 + 4) + (FIN_CHUNK + 4) * H * 4 if train else 0


def pool_step_smem(C, K, cap, train):              # launch_pool_finish
    PK = C * K if train else 0
    return C * cap * 8 + C * 16 * 8 + C * 4 * 3 + C * K * 4 + PK * (4 * 4 + 2 * H * 4) + 4 * H * 4


def fused_step_smem(C, K, D, cap):
    PK = C * K
    return (C * cap * 8 + C * 16 * 8 + C * 4 * 3 + C * K * 4 + PK * (4 * 4 + 2 * H * 4) + 4 * H * 4 + PK * 8 + 16 +
            PK * D * 4)


def tiles_step_smem(C, K, cap):
    P, CL = C * K, 64
    return (TILES_SINK + P * 32 + P * 256 * 4 + (P + 4) * 4 + P * 16 + C * cap * 8 + C * 8 + P * 8 + C * CL * 4 +
            C * 16 * 4 + C * 4 * 4 + P * 4 + P * 4 + 16 + 64)


def wide_cap(C):
    cap = 1024
    while cap > 64 and C * cap * 8 > 64 * 1024:
        cap >>= 1
    return cap


def wide_region(C, D, esz, pch):
    lists = C * wide_cap(C) * 8
    rows = pch * ((D // 16) * esz)
    return (max(lists, rows) + 15) & ~15


def wide_smem(C, K, D, esz, pch):
    PK = C * K
    return (wide_region(C, D, esz, pch) + C * 16 * 8 + C * 4 * 3 + PK * 4 + PK * 16 * 2 + PK * 8 + PK * 4 +
            (4 * H + 32) * 4 + 8 + PK * 8 + 16 + 16 * 16 + 2 * 20 * 4)


def wide_pch(C, K, D, esz):
    pch = (C * K + 31) & ~31
    while pch > WD_PCH_MIN and wide_smem(C, K, D, esz, pch) > FS_MAX_DYN_LDS:
        pch -= 32
    return max(pch, WD_PCH_MIN)


def row(C, K, D, esz, train):
    cap, pch = step_cap(C), wide_pch(C, K, D, esz)
    tiles = tiles_step_smem(C, K, cap)
    return [finish_smem(C, K, train), pool_step_smem(C, K, cap, train), fused_step_smem(C, K, D, cap), tiles,
            tiles - TILES_SINK, wide_smem(C, K, D, esz, pch), wide_region(C, D, esz, pch), pch, wide_cap(C)]


def check_anchors():
    for D in AXES["D"]:
        assert tiles_step_smem(2, 10, step_cap(2)) == 40032
    assert tiles_step_smem(15, 4, step_cap(15)) == 133240
    assert fused_step_smem(15, 4, 256, step_cap(15)) == 158420
    assert fused_step_smem(2, 10, 1024, step_cap(2)) == 110424
    assert wide_pch(61, 8, 1024, 4) == 480 and wide_smem(61, 8, 1024, 4, 480) == 160340
    assert fused_step_smem(8, 8, 256, step_cap(8)) == 167792 > FS_MAX_DYN_LDS    # why that shape takes three launches


def record():
    return {"parent": PARENT, "axes": AXES, "fields": FIELDS,
            "rows": [row(*pt) for pt in itertools.product(*AXES.values())]}


if __name__ == "__main__":
    check_anchors()
    with open(RECORD, "w") as f:
        json.dump(record(), f, separators=(",", ":"))
        f.write("\n")
    print("wrote", RECORD)
