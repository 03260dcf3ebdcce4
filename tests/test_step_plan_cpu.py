"""Which step kernel a shape gets is decided in one place (StepPlan: step_plan in moc_amd/csrc/moc_meta.hip).  moc_train_runs_mode and
moc_p2p_step_supported are pure host functions over that decision: their answers over a grid of shapes were recorded
before the decision was gathered into the plan (tests/golden/step_dispatch.json) and must not move."""
import ctypes as C
import itertools
import json
import os

from moc_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "step_dispatch.json")
AXES = {
    "C": [1, 2, 3, 8, 9, 16, 17, 30, 64, 65],
    "topk": [1, 10, 16, 17, 32],
    "D": [256, 512, 768, 1024, 1280],
    "topj": [100, 800],
    "max_rows": [16, 4096, 4097, 9000, 60000],
    "W2_alt": [1, 0],
    "tile_ws": ["exact", "short", "null"],
    "row_off_host": [1, 0],
}
N_SLIDES = 3


def tables():
    """(runs_mode, p2p): the answers as strings of digits, in itertools.product order of AXES (p2p: its four axes)"""
    lib = _lib.lib()
    # never dereferenced: both functions only test these pointers against NULL
    dummy = C.cast(C.create_string_buffer(64), C.c_void_p).value
    runs = []
    for c, k, d, j, rows, w2, tile, roh in itertools.product(*AXES.values()):
        B = _lib.MocBatch(D=d, total_rows=N_SLIDES * rows, n_slides=N_SLIDES, max_rows=rows, C=c, Ce=c, topj=j, topk=k)
        B.row_off_host = dummy if roh else None
        ws = _lib.MocMetaWs()
        ws.W2_alt = dummy if w2 else None
        if tile != "null":
            ws.tile_ws = dummy
            ws.tile_ws_bytes = lib.moc_tile_ws_bytes(B.total_rows, N_SLIDES, c) - (1 if tile == "short" else 0)
        runs.append(str(lib.moc_train_runs_mode(C.byref(B), C.byref(ws))))
    p2p = [str(lib.moc_p2p_step_supported(c, k, d, j))
           for c, k, d, j in itertools.product(AXES["C"], AXES["topk"], AXES["D"], AXES["topj"])]
    return "".join(runs), "".join(p2p)


def test_decisions_match_the_recorded_table():
    gold = json.load(open(GOLDEN))
    assert gold["axes"] == AXES and gold["n_slides"] == N_SLIDES
    runs, p2p = tables()
    assert len(gold["runs_mode"]) == len(runs) == 30000 and len(gold["p2p_step_supported"]) == len(p2p) == 500
    # every answer occurs: the grid does not pass vacuously
    assert set(gold["runs_mode"]) == {"0", "1", "2"} and set(gold["p2p_step_supported"]) == {"0", "1"}
    bad = [i for i, (a, b) in enumerate(zip(gold["runs_mode"], runs)) if a != b]
    assert not bad, "moc_train_runs_mode differs at %d grid points, first %s" % (
        len(bad), list(itertools.product(*AXES.values()))[bad[0]])
    assert p2p == gold["p2p_step_supported"]
