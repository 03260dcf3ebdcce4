"""Host orchestration over libmoc_hip: packed slide batches, the prepared
classifier bank, the meta-learner state shared with torch.optim.Adam, and the
batched phase-A / phase-B drivers.  PyTorch here is plumbing only: it owns the
device buffers and the stream; every kernel is ours.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
import weakref
from typing import Sequence

import torch

from . import _lib
from ._lib import MocBankSet, MocBatch, MocMeta, MocMetaWs, MocRuns, check, lib, ptr

HIDDEN = 64
# MOC_STEP_GRAPH=1: a pass of meta-steps as one hipGraph launch (moc_train_steps_graph) instead of 2 n + 1 stream
# launches (moc_train_steps).  Bit-identical (tests/test_gpu_graph.py) and it frees the host (38 against 170-250 us per
# 32-step pass), but on the GPU the replayed chain is 1-3 % SLOWER than the stream launches (fp32 bags: 27.7 against
# 26.9 us per step; steady state 36.6 k against 37.0 k meta-steps/s, bf16 42.5 k against 43.4 k) and its first kernel
# starts later (the whole graph is enqueued before the doorbell), so stream launches stay the default.
STEP_GRAPH = os.environ.get("MOC_STEP_GRAPH", "0") == "1"
GRAPH_TABLE_STEPS = 4096        # Adam steps of coefficients kept on the device per table build
CAND_FROM_STATS = os.environ.get("MOC_CAND_FROM_STATS", "1") != "0"   # evaluation: no materialised candidate columns (0: as in training)
COMPACT_STATS = os.environ.get("MOC_COMPACT_STATS", "1") != "0"     # wide banks: C + 5 statistics per row (0: always 2C + 3)

# The look-ahead phase A of a train pass stays off MOC_RESERVE_CUS compute units, which the sequential meta-steps of the
# pass in progress then find free (moc_batch_t.cu_reserved + tile_ticket, include/moc_hip.h; 0: the whole chip, static
# walk).  Measured on the default workload (scripts/sweep_reserve_cus.sh, profiles/NOTES.md): 0 -> 42.9 k, 48 -> 44.2 k,
# 64 -> 45.6 k, 96 -> 42.9 k meta-steps/s; the ticketed walk alone costs the score pass 7 % (fp32) / 19 % (bf16), so
# passes with nothing beside them (evaluation) keep the static walk.
RESERVE_CUS = int(os.environ.get("MOC_RESERVE_CUS", "64"))


def score_ring_mode(value):
    """MOC_SCORE_RING: which score passes ask for the LDS-DMA ring kernel (MOC_SCORES_RING, include/moc_hip.h) -- "0" none,
    "lookahead" the look-ahead phase A of a train pass (which then takes no ticket and reserves no compute units: the ring
    kernel shares every CU with the meta-steps), "all" evaluation's fp32 launches against one-n-tile banks as well."""
    v = (value or "0").strip().lower()
    if v not in ("0", "lookahead", "all"):
        raise ValueError(f"MOC_SCORE_RING={value!r}: expected 0, lookahead or all")
    return v


# Default "lookahead": bench.py --gpus 1 --steps 1600 --warmup 160, eight alternating runs in one call -- 59.3 k meta-steps/s
# (57.2-59.9) against 57.1 k (56.4-58.2) for the register kernel off 64 reserved CUs (profiles/NOTES.md, "The look-ahead
# score pass as an LDS-DMA ring").  "all" is not measured yet: alone on the chip the ring kernel is 30 % slower than the
# register kernel, so evaluation keeps the latter.
SCORE_RING = score_ring_mode(os.environ.get("MOC_SCORE_RING", "lookahead"))
# the training step pools among the forward's tile records (moc_meta_ws_t.tile_ws; 0: re-reads every mixed score, round 3)
TILE_RECORDS = os.environ.get("MOC_TILE_RECORDS", "1") != "0"
N_SEL_HOST = os.environ.get("MOC_N_SEL_HOST", "1") != "0"            # moc_batch_t.n_sel_mail / n_sel_host for the train steps (0: never, diagnostic)

# bench.py sets this to a list: every batched score-pass launch then appends
# (start_event, stop_event, algorithmic_bytes) recorded on the launch stream.
SCORE_EVENTS = None


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream():
    """The current stream's hipStream_t.  torch.cuda.current_stream() builds a Stream object through four layers of device-index
    look-ups (4-9 us a call, several calls per pass, two of them in front of a pass's first launch); the raw accessor is the
    same handle in 0.3 us."""
    if _raw_stream is not None:
        return C.c_void_p(_raw_stream(torch.cuda.current_device()))
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


_census = {}      # device index -> sorted list of (xcc, hw_id_bits) slots
_reserved = {}    # (device index, n) -> device int32[128] bitmap


def cu_slots(device):
    """The compute units of `device` as (xcc, HW_ID[15:8]) slots, found by moc_cu_census (once per process)."""
    dev = torch.device(device)
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    if idx not in _census:
        n_cu = torch.cuda.get_device_properties(idx).multi_processor_count
        found = []
        with torch.cuda.device(idx):
            for hold_us in (20, 100, 400):          # (another process may hold whole CUs for a while: look again, longer)
                hist = torch.zeros(16 * 256, dtype=torch.int32, device=dev)
                check(lib().moc_cu_census(ptr(hist), 16384, hold_us, _stream()), "moc_cu_census")
                h = hist.cpu().view(16, 256)
                found = sorted(set(found) | {(x, s) for x in range(16) for s in range(256) if int(h[x, s]) > 0})
                if len(found) >= n_cu:
                    break
        _census[idx] = found
    return _census[idx]


def reserved_cus(device, n):
    """Device bitmap (int32[128], bit xcc * 256 + HW_ID[15:8]) of `n` compute units the look-ahead score pass stays off:
    an equal share of every XCD, dealt over its shader engines / arrays (highest CU id of each first).  None for n <= 0."""
    n = int(n)
    if n <= 0:
        return None
    dev = torch.device(device)
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    key = (idx, n)
    if key not in _reserved:
        chosen = choose_reserved_slots(cu_slots(dev), n)
        if not chosen:                      # too small a device to give any compute unit away
            import warnings
            warnings.warn(f"moc_amd: {len(cu_slots(dev))} compute units visible -- the look-ahead score pass keeps the "
                          "static whole-chip walk (MOC_RESERVE_CUS ignored)")
            _reserved[key] = None
        else:
            words = reserved_words(chosen)
            t = torch.tensor([w - (1 << 32) if w >= (1 << 31) else w for w in words], dtype=torch.int32)
            _reserved[key] = t.to(dev)
    return _reserved[key]


def choose_reserved_slots(slots, n):
    """`n` of the (xcc, HW_ID[15:8]) slots: an equal share of every XCD (the first n % XCDs get one more), inside an XCD
    dealt round-robin over its shader engines / arrays (HW_ID[15:12]), the highest CU id of each first.  Pure."""
    n = int(n)
    assert n > 0, f"{n} reserved compute units"
    # a smaller part or partition (CPX / DPX, HSA_CU_MASK), or a census that saw less: never more than three quarters of
    # what exists; an empty result tells the caller to keep the static whole-chip walk
    n = min(n, len(slots) * 3 // 4)
    if n <= 0:
        return []
    xccs = sorted({x for x, _ in slots})
    chosen = []
    per = [n // len(xccs) + (1 if i < n % len(xccs) else 0) for i in range(len(xccs))]
    for x, want in zip(xccs, per):
        groups = {}
        for _, s_ in (t for t in slots if t[0] == x):
            groups.setdefault(s_ >> 4, []).append(s_)                # HW_ID[15:12] = SE | SH; [11:8] = CU
        order = [sorted(g, reverse=True) for _, g in sorted(groups.items())]
        want = min(want, sum(len(g) for g in order) * 3 // 4)      # (an incomplete census: never more than three quarters of what was seen)
        k = 0
        while want > 0:
            g = order[k % len(order)]
            if g:
                chosen.append((x, g.pop(0)))
                want -= 1
            k += 1
    return chosen


def reserved_words(chosen):
    """The 128-word bitmap moc_batch_t.cu_reserved points at: bit xcc * 256 + HW_ID[15:8]."""
    words = [0] * 128
    for x, s_ in chosen:
        assert 0 <= x < 16 and 0 <= s_ < 256
        bit = x * 256 + s_
        words[bit >> 5] |= 1 << (bit & 31)
    return words


_stream_objs = {}


def stream_obj():
    """torch's Stream object of the current stream, cached by raw handle: Event.record() / Event.wait() without a stream
    argument go through torch.cuda.current_stream(), 7-9 us a call (device-index look-ups, an availability check that reads the
    environment) -- three of them per pass, one in front of the pass's first launch."""
    if _raw_stream is None:
        return torch.cuda.current_stream()
    dev = torch.cuda.current_device()
    key = (dev, _raw_stream(dev))
    obj = _stream_objs.get(key)
    if obj is None:
        if len(_stream_objs) > 64:
            _stream_objs.clear()
        obj = _stream_objs[key] = torch.cuda.current_stream()
    return obj


def timed_scores(batch, bank):
    """moc_scores_timed on the current stream: -> (start, stop) torch events holding the score kernel's own time stamps
    (start.elapsed_time(stop) after a synchronisation = the kernel's duration as rocprofv3 reports it)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()                                   # (torch creates the HIP event at its first record)
    e1.record()
    h0, h1 = e0.cuda_event, e1.cuda_event
    assert h0 and h1, "torch did not hand out the HIP event handles"
    c = batch._score_c() if hasattr(batch, "_score_c") else batch.c
    check(lib().moc_scores_timed(C.byref(c), ptr(bank.image), _stream(), C.c_void_p(h0), C.c_void_p(h1)), "moc_scores_timed")
    return e0, e1


def _dtype_code(dt: torch.dtype) -> int:
    if dt == torch.float32:
        return _lib.MOC_F32
    if dt == torch.bfloat16:
        return _lib.MOC_BF16
    if dt == torch.float16:
        return _lib.MOC_F16
    raise AssertionError(f"bag dtype {dt} unsupported (float32, bfloat16 or float16)")


class Bank:
    """The classifier bank [zeroshot_weights | zeroshot_weights_ext[:, C:]] re-laid
    for the score kernel (moc_prepare_bank).  Cached per (tensors, versions, dtype)."""

    _cache: dict = {}

    def __init__(self, W: torch.Tensor, W_ext: torch.Tensor, dtype: torch.dtype, device, fg_from_ext=False):
        assert W.dim() == 2 and W_ext.dim() == 2 and W.size(0) == W_ext.size(0)
        assert W_ext.size(1) > W.size(1), "logits should have more bg classes"
        self.D, self.C, self.Ce = W.size(0), W.size(1), W_ext.size(1)
        self.dtype = dtype
        Wd = W.detach().to(device=device, dtype=torch.float32).contiguous()
        Wed = W_ext.detach().to(device=device, dtype=torch.float32).contiguous()
        code = _dtype_code(dtype)
        nbytes = lib().moc_bank_bytes(self.D, self.Ce, code)
        self.image = torch.empty(nbytes, dtype=torch.uint8, device=device)
        check(lib().moc_prepare_bank(ptr(Wd), ptr(Wed), self.D, self.C, self.Ce, code, int(fg_from_ext),
                                     ptr(self.image), _stream()), "moc_prepare_bank")
        self._keep = (Wd, Wed)

    @classmethod
    def get(cls, W, W_ext, dtype, device, fg_from_ext=False) -> "Bank":
        device = torch.device(device)
        key = (W.data_ptr(), W._version, tuple(W.shape), W_ext.data_ptr(), W_ext._version,
               tuple(W_ext.shape), dtype, str(device), bool(fg_from_ext))
        hit = cls._cache.get(key)
        if hit is None:
            if len(cls._cache) > 16:
                cls._cache.clear()
            hit = cls._cache[key] = (cls(W, W_ext, dtype, device, fg_from_ext), W, W_ext)
        return hit[0]


BANK_SET_MAX_CE = 16        # a bank of a BankSet is ONE n-tile of the score kernel's image


def plan_bank_passes(D: int, dtype: torch.dtype, n_banks: int):
    """The cuts of `n_banks` narrow banks into score passes: [(first bank, banks), ...], each of at most
    moc_scores_banks_max(D, storage) banks, in order.  Pure (the limit is host arithmetic of the library: no GPU)."""
    per = int(lib().moc_scores_banks_max(int(D), _dtype_code(dtype)))
    assert per >= 1, f"no multi-bank score pass at D={D} on {dtype} bags (one bank's image does not fit in LDS)"
    assert n_banks >= 1, "no bank given"
    return [(g0, min(per, n_banks - g0)) for g0 in range(0, n_banks, per)]


def bank_work_row_bytes(C_: int) -> int:
    """Bytes per bag row of ONE bank's work arrays (SlideBatch.scores_banks: stats, sel_flag, sel_idx, sel_row, cand, and the
    mixed scores of the evaluation forward) -- what a chunk of slides costs per bank beside the bags themselves."""
    return 4 * (2 * C_ + 3) + 1 + 4 + 8 + 4 * (2 * C_ + 2) + 4 * C_


class BankSet:
    """Several classifier banks of one class count, each at most 16 columns wide, as moc_scores_banks takes them: bank g's
    image (moc_prepare_bank with its own Ce and fg_from_ext) at g * moc_bank_bytes(D, 16, storage) of one array, and the
    list cut into passes of at most moc_scores_banks_max banks (plan_bank_passes).
    banks: [(W [D, C], W_ext [D, Ce][, fg_from_ext]), ...]."""

    def __init__(self, banks, dtype: torch.dtype, device):
        banks = [tuple(b) for b in banks]
        assert banks and all(len(b) in (2, 3) for b in banks), "BankSet: a list of (W, W_ext[, fg_from_ext])"
        W0 = banks[0][0]
        self.D, self.C, self.dtype = int(W0.size(0)), int(W0.size(1)), dtype
        self.Ce = []
        for g, b in enumerate(banks):
            W, We = b[0], b[1]
            assert W.dim() == 2 and We.dim() == 2 and W.size(0) == self.D and We.size(0) == self.D, f"BankSet: bank {g}: bad shapes"
            assert W.size(1) == self.C, f"BankSet: banks of different C ({self.C} and {W.size(1)} classes) do not share a pass"
            assert We.size(1) > self.C, "logits should have more bg classes"
            assert We.size(1) <= BANK_SET_MAX_CE, \
                f"BankSet: bank {g} has Ce={We.size(1)} > {BANK_SET_MAX_CE} columns; wide banks keep zs_evaluation / evaluation per bank"
            self.Ce.append(int(We.size(1)))
        self.n_banks = len(banks)
        self.passes = plan_bank_passes(self.D, dtype, self.n_banks)
        code = _dtype_code(dtype)
        self.tile_bytes = int(lib().moc_bank_bytes(self.D, BANK_SET_MAX_CE, code))
        assert lib().moc_bank_set_bytes(self.D, self.n_banks, code) == self.n_banks * self.tile_bytes
        self.image = torch.empty(self.n_banks * self.tile_bytes, dtype=torch.uint8, device=device)
        self._keep = []
        for g, b in enumerate(banks):
            Wd = b[0].detach().to(device=device, dtype=torch.float32).contiguous()
            Wed = b[1].detach().to(device=device, dtype=torch.float32).contiguous()
            check(lib().moc_prepare_bank(ptr(Wd), ptr(Wed), self.D, self.C, self.Ce[g], code, int(bool(b[2])) if len(b) == 3 else 0,
                                         self.image.data_ptr() + g * self.tile_bytes, _stream()), "moc_prepare_bank")
            self._keep.append((Wd, Wed))


class SlideBatch:
    """Slides packed back to back in one device array + every work array of phase A.

    X: [total_rows, D] device tensor (float32 or bfloat16); sizes: rows per slide.
    mask: optional bool/uint8 [total_rows] keep flags (host or device)."""

    def __init__(self, X: torch.Tensor, sizes: Sequence[int], C_: int, Ce: int, topj: int, topk: int,
                 discard=(), mask: torch.Tensor | None = None, x_starts: Sequence[int] | None = None):
        assert X.is_cuda and X.dim() == 2 and X.is_contiguous()
        sizes = [int(s) for s in sizes]
        assert len(sizes) > 0 and min(sizes) > 0, "empty slide"
        if x_starts is None:
            assert sum(sizes) == X.size(0), "sizes must partition X's rows"
        else:
            assert len(x_starts) == len(sizes) and all(0 <= st and st + n <= X.size(0) for st, n in zip(x_starts, sizes))
        dev = X.device
        self.X, self.sizes, self.device = X, sizes, dev
        self.n_slides, self.total, self.D = len(sizes), sum(sizes), X.size(1)
        self.C, self.Ce, self.topj, self.topk = int(C_), int(Ce), int(topj), int(topk)
        self.discard_bits = _lib.discard_bits(discard)
        off = [0]
        for s in sizes:
            off.append(off[-1] + s)
        self.row_off_host = off
        self._row_off_c = (C.c_int64 * len(off))(*off)        # host copy handed to the C ABI
        self.row_off = torch.tensor(off, dtype=torch.int64).to(dev, non_blocking=True)
        self.x_off = None
        if x_starts is not None:
            self.x_off = torch.tensor([int(v) for v in x_starts], dtype=torch.int64).to(dev, non_blocking=True)
        T, n = self.total, self.n_slides
        self.mask = None
        self.kept_rows_host = T          # rows the score pass has to read (algorithmic)
        if mask is not None:
            assert mask.numel() == T
            if not mask.is_cuda:
                self.kept_rows_host = int(mask.sum())
            self.mask = mask.to(torch.uint8).to(dev, non_blocking=True).contiguous()
        i32 = dict(dtype=torch.int32, device=dev)
        self.kept = torch.empty(T + 16, **i32) if mask is not None else None   # +16: see moc_hip.h
        self.n_kept = torch.empty(n, **i32) if mask is not None else None
        self.stats = torch.empty((2 * self.C + 3, T), dtype=torch.float32, device=dev)
        self.sel_flag = torch.empty(T, dtype=torch.uint8, device=dev)
        self.sel_idx = torch.empty(T, **i32)
        self.sel_row = torch.empty(T, dtype=torch.int64, device=dev)
        self.n_sel = torch.empty(n, **i32)
        self.cand = torch.empty((2 * self.C + 2, T), dtype=torch.float32, device=dev)
        self.c = MocBatch(
            X=ptr(X), dtype=_dtype_code(X.dtype), D=self.D, total_rows=T, n_slides=n, max_rows=max(sizes),
            row_off=ptr(self.row_off), row_off_host=C.cast(self._row_off_c, C.c_void_p), x_off=ptr(self.x_off),
            mask=ptr(self.mask), C=self.C, Ce=self.Ce, topj=self.topj,
            topk=self.topk, discard_bits=self.discard_bits, flags=0, kept=ptr(self.kept),
            n_kept=ptr(self.n_kept), stats=ptr(self.stats), sel_flag=ptr(self.sel_flag),
            sel_idx=ptr(self.sel_idx), sel_row=ptr(self.sel_row), n_sel=ptr(self.n_sel), cand=ptr(self.cand))
        self.ticket = None
        self.cu_reserved = None
        self._ws = None
        self.stats_cache = None          # (statistics of every row of X, layout flag): phase A copies instead of reading the bags
        # moc_batch_t.n_sel_mail: a pinned mailbox of one 64-bit word per slide, (ticket << 32) | S, which compact_kernel's
        # workgroup of the slide stores beside n_sel[b]; the C step loop reads slide b's word in front of step b's two
        # launches -- where it carries this batch's current ticket the forward takes S as an argument instead of loading
        # it, launches exactly the workgroups that have rows, and the step reads fewer record keys per lane; where it has
        # not arrived the step runs on the device count.  Every phase A takes a fresh ticket (_n_sel_stale), so the words
        # of an earlier one never pass.  Masked (training) batches only.  The mailbox lives as long as the batch.
        self._n_sel_mail = torch.zeros(n, dtype=torch.int64).pin_memory() if (N_SEL_HOST and mask is not None) else None
        self._n_sel_ticket = 0
        self._n_sel_pin = self._n_sel_ev = None    # (the batched runs' copy of all counts at once: _n_sel_request)

    def reserve_cus(self, n: int | None = None, ticket: bool | None = None):
        """This batch's score passes stay off `n` compute units (default MOC_RESERVE_CUS) and hand their tiles out by
        ticket: for a phase A that runs beside the meta-steps of another pass.  0 undoes it (static walk, whole chip);
        ticket=True with n = 0: the ticketed walk alone (tests)."""
        n = RESERVE_CUS if n is None else int(n)
        use_ticket = (n > 0) if ticket is None else bool(ticket)
        assert use_ticket or n <= 0, "reserved compute units need the ticketed walk"
        self.cu_reserved = reserved_cus(self.device, n) if n > 0 else None
        if n > 0 and self.cu_reserved is None and ticket is None:
            use_ticket = False                  # nothing could be reserved on this device: static walk, whole chip
        if use_ticket and self.ticket is None:
            self.ticket = torch.zeros(_lib.TICKET_WORDS, dtype=torch.int32, device=self.device)
        self.c.tile_ticket = ptr(self.ticket) if use_ticket else None
        self.c.cu_reserved = ptr(self.cu_reserved)

    def use_score_ring(self, on: bool = True):
        """This batch's score passes ask for the ring kernel (MOC_SCORES_RING): no ticket, no reserved compute units.
        -> whether moc_scores gives the batch that kernel (fp32 bags, one n-tile, LDS for at least three ring slots); where
        it does not, the bit is cleared again (static walk, whole chip, until reserve_cus says otherwise).  on=False clears it."""
        if on:
            self.reserve_cus(0)
            self.c.flags |= _lib.MOC_SCORES_RING
            if lib().moc_scores_form(C.byref(self.c)) == _lib.SCORE_FORM_RING:
                return True
        self.c.flags &= ~_lib.MOC_SCORES_RING
        return False

    def lookahead(self):
        """For a phase A that runs beside the meta-steps of another pass.  The batch takes the ticket array and the reserved
        compute units of the register kernel (reserve_cus) either way; where MOC_SCORE_RING asks for the ring kernel and the
        batch can have it, its score launches go out WITHOUT them and with the ring bit (_score_c) -- the ring kernel shares
        every CU with the steps.  A caller that takes the ticket off the batch (bench.py's `whole_chip` figure) gets the
        register kernel's static walk, as before."""
        self.reserve_cus()
        self._ring_lookahead = False
        if SCORE_RING != "0":
            if self.c.tile_ticket is None:
                self.use_score_ring()                 # (nothing could be reserved on this device: the bit in the batch itself)
            else:
                self._ring_lookahead = True
                self._ring_lookahead = lib().moc_scores_form(C.byref(self._score_c())) == _lib.SCORE_FORM_RING

    _ring_lookahead = False

    def _score_c(self):
        """The moc_batch_t a score launch gets: the batch's own, or for a look-ahead batch in ring mode a copy with
        MOC_SCORES_RING and neither ticket nor reserved set."""
        if not self._ring_lookahead or self.c.tile_ticket is None:
            return self.c
        v = MocBatch.from_buffer_copy(self.c)
        v.flags |= _lib.MOC_SCORES_RING
        v.tile_ticket = v.cu_reserved = None
        return v

    def set_mask(self, host_mask_u8: torch.Tensor, kept_rows: int):
        """New keep flags for the same visits (next epoch): async H2D into the resident mask array."""
        assert self.mask is not None and host_mask_u8.numel() == self.total and host_mask_u8.dtype == torch.uint8
        self.mask.copy_(host_mask_u8, non_blocking=True)
        self.c.mask = ptr(self.mask)
        self.kept_rows_host = int(kept_rows)
        self.c.max_rows = max(self.sizes)       # (use_host_mask may have tightened it to ANOTHER mask's kept rows)

    def use_host_mask(self, pinned_mask_u8: torch.Tensor, kept_rows: int, max_kept: int | None = None):
        """Keep flags read by the compaction kernel straight from PINNED host memory (device-mapped by
        hipHostMalloc): no copy command at all.  Measured on the GPU box: the 480 KB asynchronous upload it
        replaces blocked the issuing thread for ~7 ms once every few dozen epochs (scripts/diag_stall.py).
        The caller keeps the buffer untouched until the pass that reads it has run."""
        assert pinned_mask_u8.is_pinned() and pinned_mask_u8.numel() == self.total and pinned_mask_u8.dtype == torch.uint8
        self._host_mask = pinned_mask_u8
        self.c.mask = pinned_mask_u8.data_ptr()
        self.kept_rows_host = int(kept_rows)
        # the flags are host bytes: the exact largest kept-row count of any slide is a tighter max_rows than the bag
        # sizes (about half) -- it sizes the grids of everything after the compaction and decides kernel shapes
        mk = max_kept if max_kept is not None else \
            int(lib().moc_host_max_kept(pinned_mask_u8.data_ptr(), C.cast(self._row_off_c, C.c_void_p), self.n_slides))
        assert 0 <= mk <= max(self.sizes)
        self.c.max_rows = max(1, mk)

    # ---- phase A ----
    def _layout(self, compact: bool, cand_from_stats: bool = False):
        """Statistics layout of the next score pass and of what reads it (include/moc_hip.h MOC_STATS_COMPACT);
        cand_from_stats: an evaluation pass -- the forward reads the candidate scores from the statistics, the
        [2C+2, S] candidate columns of wide banks are never written (MOC_CAND_FROM_STATS)."""
        ring = self.c.flags & _lib.MOC_SCORES_RING
        if SCORE_RING == "all" and self.c.dtype == _lib.MOC_F32 and self.Ce <= 16 and not self.c.tile_ticket and not self.c.cu_reserved:
            ring = _lib.MOC_SCORES_RING            # (shapes the ring kernel does not cover keep their kernels: moc_scores_plan.h)
        self.c.flags = ((_lib.MOC_STATS_COMPACT if compact else 0) | (_lib.MOC_CAND_FROM_STATS if cand_from_stats else 0) | ring |
                        (self.c.flags & (_lib.MOC_SELECT_PER_COLUMN | _lib.MOC_FORWARD_ROWS64 | _lib.MOC_FORWARD_FOUR_WAVES | _lib.MOC_FORWARD_ROWS16)))

    def _eval_layout(self, compact: bool):
        """The layout of an evaluation pass -- only meta_forward follows (no train step, no ablation mix): candidates
        straight from the statistics."""
        self._layout(compact, cand_from_stats=CAND_FROM_STATS and self.C > 4)

    def phase_a(self, bank: Bank, for_eval: bool = False):
        assert bank.D == self.D and bank.C == self.C and bank.Ce == self.Ce and bank.dtype == self.X.dtype
        # wide banks: C + 5 statistics per row instead of 2C + 3 (the selector and the candidate gather re-form the
        # softmax columns); phase A is the only reader of its own statistics, so the layout is its private choice.
        (self._eval_layout if for_eval else self._layout)(COMPACT_STATS and self.Ce > 16)
        self._n_sel_stale()
        if SCORE_EVENTS is None and self.stats_cache is None:
            check(lib().moc_phase_a(C.byref(self._score_c()), ptr(bank.image), _stream()), "moc_phase_a")
            return
        # same four launches, with events around the score pass
        check(lib().moc_mask_compact(C.byref(self.c), _stream()), "moc_mask_compact")
        self.phase_a_tail(bank)

    _n_sel_mail = None                  # (class defaults: CompactBatch builds its own fields)
    _n_sel_ticket = 0
    _n_sel_pin = None
    _n_sel_ev = None

    def _n_sel_stale(self):
        """n_sel is about to be rewritten: no host copy describes it any more, and the mailbox words of the launch that
        rewrites it travel under a fresh ticket (from 1; 0, "none", is skipped on wrap)."""
        self.c.n_sel_host = None
        self._n_sel_ev = None
        if self._n_sel_mail is None:
            return
        self._n_sel_ticket = (self._n_sel_ticket + 1) & 0xFFFFFFFF or 1
        self.c.n_sel_mail, self.c.n_sel_ticket = ptr(self._n_sel_mail), self._n_sel_ticket

    def _n_sel_request(self):
        """The batched runs (moc_amd.runs), whose lockstep launches want every run's count or none: behind the launches that
        write n_sel, on their stream, the asynchronous copy of all counts into a pinned buffer and its event."""
        if self._n_sel_mail is None:
            return
        if self._n_sel_pin is None:
            self._n_sel_pin = torch.empty(self.n_slides, dtype=torch.int32).pin_memory()
        self.c.n_sel_host = None
        self._n_sel_pin.copy_(self.n_sel, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(stream_obj())
        self._n_sel_ev = ev

    def publish_n_sel(self, allow: bool = True):
        """Called in front of the train steps: hands them the mailbox and the ticket its words must carry (allow), or
        nothing at all; -> whether there is a mailbox to hand over.  No event is queried or waited for: the C step loop looks at
        a slide's word when it issues that slide's step (and waits for the first one's, MOC_N_SEL_SPIN_US at the most).
        (A copy of all counts that _n_sel_request has queued is handed over as moc_batch_t.n_sel_host once its event has
        completed.)"""
        ev = self._n_sel_ev
        self.c.n_sel_host = ptr(self._n_sel_pin) if (allow and ev is not None and ev.query()) else None
        ok = allow and self._n_sel_mail is not None
        self.c.n_sel_mail, self.c.n_sel_ticket = (ptr(self._n_sel_mail), self._n_sel_ticket) if ok else (None, 0)
        return ok

    def phase_a_head(self, bank: Bank):
        """The first launch of phase A alone -- the kept-row lists from the keep flags (read over PCIe when they are host
        flags) -- for a caller that runs it ahead of the rest (moc_amd.runs)."""
        assert bank.D == self.D and bank.C == self.C and bank.Ce == self.Ce and bank.dtype == self.X.dtype
        self._layout(COMPACT_STATS and self.Ce > 16)
        self._n_sel_stale()
        check(lib().moc_mask_compact(C.byref(self.c), _stream()), "moc_mask_compact")

    def phase_a_tail(self, bank: Bank):
        """... and the rest: score pass (timed when bench.py collects SCORE_EVENTS), selection, union, candidates."""
        if self.stats_cache is not None:
            # opt-in (include/moc_hip.h moc_scores_from_cache): the kept rows' statistics from those of an earlier, unmasked
            # score pass over the same rows and bank -- the same bits, no read of the bags
            cache, compact = self.stats_cache
            assert compact == bool(self.c.flags & _lib.MOC_STATS_COMPACT) and cache.size(1) == self.X.size(0)
            check(lib().moc_scores_from_cache(C.byref(self.c), ptr(cache), cache.size(1), _stream()), "moc_scores_from_cache")
        elif SCORE_EVENTS is None:
            check(lib().moc_scores(C.byref(self._score_c()), ptr(bank.image), _stream()), "moc_scores")
        else:
            e0, e1 = timed_scores(self, bank)
            SCORE_EVENTS.append((e0, e1, self.kept_rows_host * self.D * self.X.element_size()))
        self._n_sel_stale()
        self.select()
        self.gather_candidates()

    def scores(self, bank: Bank):
        self._layout(False)                      # callers of scores() read `stats` themselves: the full layout
        check(lib().moc_mask_compact(C.byref(self.c), _stream()), "moc_mask_compact")
        check(lib().moc_scores(C.byref(self.c), ptr(bank.image), _stream()), "moc_scores")

    def scores_banks(self, bank_set: "BankSet"):
        """The score pass for every bank of `bank_set` in one read of the bags per group of banks (moc_scores_banks): -> one
        light batch per bank (BankView) that shares this batch's X, layout and mask lists and owns its statistics, flags,
        selection and candidate arrays, with its bank's C and Ce -- bit for bit what scores(bank) leaves in a batch of that
        bank alone; moc_select, moc_gather_candidates, moc_meta_forward, moc_topk_mean_multi and moc_pool_loss run on it
        unchanged.  The views are kept with this batch and handed out again for a set of the same (C, Ce) list."""
        assert bank_set.D == self.D and bank_set.dtype == self.X.dtype, "scores_banks: the bank set is for another D / storage"
        assert self.c.tile_ticket is None and self.c.cu_reserved is None, "scores_banks: an evaluation pass (static walk, whole chip)"
        key = (bank_set.C, tuple(bank_set.Ce))
        if getattr(self, "_bank_views_key", None) != key:
            self._bank_views = [BankView(self, bank_set.C, ce) for ce in bank_set.Ce]
            self._bank_views_key = key
        views = self._bank_views
        check(lib().moc_mask_compact(C.byref(self.c), _stream()), "moc_mask_compact")
        c = MocBatch.from_buffer_copy(self.c)
        c.flags = 0                                   # (a cached plan's batch may carry the layout of its last phase A)
        for g0, n in bank_set.passes:
            S = MocBankSet(n_banks=n, C=bank_set.C, image=bank_set.image.data_ptr() + g0 * bank_set.tile_bytes)
            for i in range(n):
                S.Ce[i], S.stats[i], S.sel_flag[i] = bank_set.Ce[g0 + i], ptr(views[g0 + i].stats), ptr(views[g0 + i].sel_flag)
            check(lib().moc_scores_banks(C.byref(c), C.byref(S), _stream()), "moc_scores_banks")
        for v in views:
            v.c.mask, v.c.max_rows = self.c.mask, self.c.max_rows
            v._layout(False)
            v._n_sel_stale()
        return views

    def scores_for_eval(self, bank: Bank):
        """The evaluation layout, the kept-row lists and the score pass, nothing else: the first two launches of
        phase_a(for_eval=True) as two entries -- for a caller that selects several times over one set of statistics."""
        self._eval_layout(COMPACT_STATS and self.Ce > 16)
        self._n_sel_stale()
        check(lib().moc_mask_compact(C.byref(self.c), _stream()), "moc_mask_compact")
        check(lib().moc_scores(C.byref(self.c), ptr(bank.image), _stream()), "moc_scores")

    def select_for_eval(self, topj: int | None = None, discard=(), clear: bool = False):
        """Over statistics that exist, in the layout they were written in: the evaluation layout, the selection and the
        candidates -- the rest of phase_a(for_eval=True) behind a score pass.  topj given: select with that topj and
        discard set instead of the batch's (see borrowed).  clear: the flags an earlier selection over these statistics
        left are cleared first (the selectors only SET flags; the score pass cleared them for the first)."""
        self._eval_layout(bool(self.c.flags & _lib.MOC_STATS_COMPACT))
        if topj is not None:
            self.c.topj, self.c.discard_bits = topj, _lib.discard_bits(discard)
        if clear:
            self.sel_flag.zero_()
        self.select()
        self.gather_candidates()

    @contextlib.contextmanager
    def borrowed(self):
        """For a caller that changes the topj, discard set or layout of a batch it does not own (a cached plan's): they
        are what they were afterwards."""
        keep = (self.c.topj, self.c.discard_bits, self.c.flags)
        try:
            yield self
        finally:
            self.c.topj, self.c.discard_bits, self.c.flags = keep
            self._n_sel_stale()

    def select(self):
        self._n_sel_stale()
        check(lib().moc_select(C.byref(self.c), _stream()), "moc_select")

    def gather_candidates(self, with_feat=False):
        feat = torch.empty((self.total, self.D), dtype=self.X.dtype, device=self.device) if with_feat else None
        check(lib().moc_gather_candidates(C.byref(self.c), ptr(feat), _stream()), "moc_gather_candidates")
        return feat

    # ---- phase B work arrays ----
    def meta_ws(self):
        if self._ws is None:
            dev, T, n, Cc, K = self.device, self.total, self.n_slides, self.C, self.topk
            f32 = dict(dtype=torch.float32, device=dev)
            i32 = dict(dtype=torch.int32, device=dev)
            # (eval_only: a batch that only ever runs the evaluation forward -- H1 and the gates, 272 bytes per row that only
            # the backward pass reads, are not allocated; the forward is then always called without them)
            hidden = not getattr(self, "eval_only", False)
            t = dict(
                H1=torch.empty((T, HIDDEN), **f32) if hidden else None, gates=torch.empty((T, 4), **f32) if hidden else None,
                mixed=torch.empty((Cc, T), **f32), pooled=torch.empty((n, Cc), **f32),
                topk_idx=torch.empty((n, Cc, K), **i32), topk_cnt=torch.empty((n, Cc), **i32),
                loss=torch.empty(n, **f32), pred=torch.empty(n, **i32),
                pair_dh=torch.empty((Cc * K, HIDDEN), **f32),
                W2_alt=torch.empty((4, HIDDEN), **f32),
                pair_row=torch.empty(Cc * K, dtype=torch.int64, device=dev), n_pair=torch.zeros(1, **i32))
            # tile records (include/moc_hip.h moc_meta_ws_t.tile_ws): what the training forward leaves for the step kernel
            # (only where the tile-record step can run -- narrow banks -- and only for batches that train: masked ones and
            # the gathered batches of the exact-sequential mode; an evaluation batch of 3 M rows x 30 classes would carry 1 GB)
            trains = self.mask is not None or isinstance(self, CompactBatch)
            nb = lib().moc_tile_ws_bytes(T, n, Cc) if (TILE_RECORDS and trains and Cc <= 16 and K <= 16 and Cc * K <= 64) else 0
            t["tile_ws"] = torch.empty(nb, dtype=torch.uint8, device=dev) if nb else None
            self._ws = (t, MocMetaWs(**{k: ptr(v) for k, v in t.items()}, tile_ws_bytes=nb))
        return self._ws


class BankView(SlideBatch):
    """One bank's batch behind SlideBatch.scores_banks: the parent's X, slide layout and mask lists (shared, not copied), and
    its own statistics, flags, selection and candidate arrays with this bank's C and Ce.  An evaluation batch: no H1 / gates."""

    eval_only = True

    def __init__(self, parent: SlideBatch, C_: int, Ce: int):
        dev, T, n = parent.device, parent.total, parent.n_slides
        self.parent = parent
        self.X, self.sizes, self.device = parent.X, parent.sizes, dev
        self.n_slides, self.total, self.D = n, T, parent.D
        self.C, self.Ce, self.topj, self.topk = int(C_), int(Ce), parent.topj, parent.topk
        self.discard_bits = parent.discard_bits
        self.row_off_host, self._row_off_c, self.row_off, self.x_off = parent.row_off_host, parent._row_off_c, parent.row_off, parent.x_off
        self.mask, self.kept, self.n_kept, self.kept_rows_host = parent.mask, parent.kept, parent.n_kept, parent.kept_rows_host
        i32 = dict(dtype=torch.int32, device=dev)
        self.stats = torch.empty((2 * self.C + 3, T), dtype=torch.float32, device=dev)
        self.sel_flag = torch.empty(T, dtype=torch.uint8, device=dev)
        self.sel_idx = torch.empty(T, **i32)
        self.sel_row = torch.empty(T, dtype=torch.int64, device=dev)
        self.n_sel = torch.empty(n, **i32)
        self.cand = torch.empty((2 * self.C + 2, T), dtype=torch.float32, device=dev)
        self.c = MocBatch.from_buffer_copy(parent.c)
        self.c.C, self.c.Ce, self.c.flags = self.C, self.Ce, 0
        self.c.stats, self.c.sel_flag, self.c.sel_idx = ptr(self.stats), ptr(self.sel_flag), ptr(self.sel_idx)
        self.c.sel_row, self.c.n_sel, self.c.cand = ptr(self.sel_row), ptr(self.n_sel), ptr(self.cand)
        self.c.n_sel_host = None
        self.c.n_sel_mail, self.c.n_sel_ticket = None, 0      # (the parent's mailbox holds the PARENT's counts)
        self.ticket = self.cu_reserved = None
        self._ws = None
        self.stats_cache = None


def build_stats_cache(X: torch.Tensor, sizes, starts, bank: "Bank", topj: int, topk: int):
    """The statistics of EVERY row of X (one unmasked score pass over the slides `sizes` at rows `starts`, which must cover
    what later passes visit) -> (stats_all [rows of stats, X rows] indexed by the row's position in X, compact flag) -- what
    SlideBatch.stats_cache takes.  28 bytes per row at two classes."""
    tmp = SlideBatch(X, sizes, bank.C, bank.Ce, topj, topk, (), x_starts=starts)
    compact = COMPACT_STATS and bank.Ce > 16
    tmp._layout(compact)
    check(lib().moc_mask_compact(C.byref(tmp.c), _stream()), "moc_mask_compact")
    check(lib().moc_scores(C.byref(tmp.c), ptr(bank.image), _stream()), "moc_scores")
    ns = (bank.C + 5) if compact else (2 * bank.C + 3)
    out = torch.zeros((ns, X.size(0)), dtype=torch.float32, device=X.device)
    off = tmp.row_off_host
    for b, (st, n) in enumerate(zip(starts, sizes)):      # slot order of an unmasked pass = row order of the slide
        out[:, st:st + n] = tmp.stats[:ns, off[b]:off[b] + n]
    return out, compact


class CompactBatch(SlideBatch):
    """Phase A's RESULT for n slides with no bag behind it: the selected rows themselves (`X` [rows, D]), their
    candidate scores (`cand` [2C+2, rows]) and `n_sel` [n] -- what moc_pack_selected_rows writes on every rank and
    the exact-sequential multi-GPU mode all-gathers (dist.train_seq).  The phase-B entry points take it like any
    batch: sel_row is the identity, slide b's rows are X[row_off[b] : row_off[b] + n_sel[b]] -- and row_off is set
    per pass (set_layout): the gathered pieces are as long as the pass's selections make them."""

    def __init__(self, n_slides: int, rows: int, cap: int, D: int, dtype: torch.dtype, C_: int, Ce: int, topj: int, topk: int,
                 device, X: torch.Tensor | None = None):
        T = int(rows)
        self.device, self.n_slides, self.total, self.D = device, int(n_slides), T, int(D)
        self.C, self.Ce, self.topj, self.topk, self.cap = int(C_), int(Ce), int(topj), int(topk), int(cap)
        self.sizes = [cap] * n_slides
        self.X = X if X is not None else torch.zeros((T, D), dtype=dtype, device=device)
        assert tuple(self.X.shape) == (T, D) and self.X.dtype == dtype
        self.cand = torch.zeros((2 * self.C + 2, T), dtype=torch.float32, device=device)
        self.n_sel = torch.zeros(n_slides, dtype=torch.int32, device=device)
        self.sel_row = torch.arange(T, dtype=torch.int64, device=device)
        self.row_off_host = [0] * (n_slides + 1)
        self._row_off_c = (C.c_int64 * (n_slides + 1))()
        self._row_off_pin = torch.zeros(n_slides + 1, dtype=torch.int64)
        if torch.device(device).type == "cuda":
            self._row_off_pin = self._row_off_pin.pin_memory()
        self.row_off = torch.zeros(n_slides + 1, dtype=torch.int64, device=device)
        self.discard_bits, self.mask, self.kept_rows_host = 0, None, T
        self.c = MocBatch(
            X=ptr(self.X), dtype=_dtype_code(dtype), D=self.D, total_rows=T, n_slides=self.n_slides, max_rows=cap,
            row_off=ptr(self.row_off), row_off_host=C.cast(self._row_off_c, C.c_void_p), x_off=None, mask=None,
            C=self.C, Ce=self.Ce, topj=self.topj, topk=self.topk, discard_bits=0, flags=0, kept=None, n_kept=None,
            stats=None, sel_flag=None, sel_idx=None, sel_row=ptr(self.sel_row), n_sel=ptr(self.n_sel), cand=ptr(self.cand))
        self._ws = None

    def set_layout(self, row_off):
        """First row of every slide (+ the end) for the pass whose pieces were just gathered: host copy for the kernel
        arguments of the single-slide launches, device copy (stream-ordered, from a pinned buffer the caller does not
        touch again before this set's steps have run) for the kernels that read row_off themselves."""
        assert len(row_off) == self.n_slides + 1 and row_off[-1] <= self.total
        self.row_off_host = [int(v) for v in row_off]
        for i, v in enumerate(self.row_off_host):
            self._row_off_c[i] = v
        self._row_off_pin.copy_(torch.tensor(self.row_off_host, dtype=torch.int64))
        self.row_off.copy_(self._row_off_pin, non_blocking=True)


def pack_selected(batch: SlideBatch, slide0: int, n: int, cap: int, feat_out: torch.Tensor, cand_out: torch.Tensor):
    """moc_pack_selected: slides [slide0, slide0+n) of `batch` (phase A done) -> feat_out [n, cap, D], cand_out [n, 2C+2, cap]."""
    assert feat_out.is_contiguous() and cand_out.is_contiguous() and feat_out.dtype == batch.X.dtype
    assert feat_out.numel() >= n * cap * batch.D and cand_out.numel() >= n * (2 * batch.C + 2) * cap
    check(lib().moc_pack_selected(C.byref(batch.c), slide0, n, cap, ptr(feat_out), ptr(cand_out), _stream()), "moc_pack_selected")


def pack_selected_rows(batch: SlideBatch, slide0: int, n: int, cap: int, feat_out: torch.Tensor, cand_out: torch.Tensor):
    """moc_pack_selected_rows: slides [slide0, slide0+n) of `batch` (phase A done), unpadded -> feat_out [rows, D] (slide
    b's rows behind those of the slides before it), cand_out [rows, 2C+2] row-major."""
    assert feat_out.is_contiguous() and cand_out.is_contiguous() and feat_out.dtype == batch.X.dtype
    rows = feat_out.size(0)
    assert feat_out.size(1) == batch.D and tuple(cand_out.shape) == (rows, 2 * batch.C + 2)
    check(lib().moc_pack_selected_rows(C.byref(batch.c), slide0, n, cap, ptr(feat_out), ptr(cand_out), rows, _stream()),
          "moc_pack_selected_rows")


class MetaState:
    """Views of a senet's parameters and its torch.optim.Adam state as the C ABI
    wants them.  The tensors are the optimizer's own (updated in place), so
    `optimizer.state_dict()` / `model.state_dict()` stay what the reference saves
    (main_moc.py:628)."""

    def __init__(self, model, optimizer=None, need_grads=False, bag_dtype=torch.bfloat16):
        lin1, lin2 = model.model[0], model.model[2]
        self.params = [lin1.weight, lin1.bias, lin2.weight, lin2.bias]
        assert lin1.out_features == HIDDEN and lin2.out_features == 4 and lin2.in_features == HIDDEN
        for p in self.params:
            assert p.is_cuda and p.dtype == torch.float32 and p.is_contiguous(), "senet must be fp32 on the GPU"
        self.D = lin1.in_features
        self.optimizer = optimizer
        self._group, self._graph, self._graph_ws, self._graph_ok = None, None, None, False
        kw = dict(lr=0.0, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, H=HIDDEN, D=self.D, step=0)
        names = ("W1", "b1", "W2", "b2")
        ptrs = {n: ptr(p.data) for n, p in zip(names, self.params)}
        self.grads = None
        self._state_refs = []
        if optimizer is not None:
            assert isinstance(optimizer, torch.optim.Adam), "the fused step implements torch.optim.Adam only"
            groups = [g for g in optimizer.param_groups if any(p is q for p in g["params"] for q in self.params)]
            assert len(groups) == 1, "senet parameters must sit in one param group"
            g = self._group = groups[0]
            assert not g.get("amsgrad", False) and not g.get("maximize", False), "amsgrad/maximize unsupported"
            steps = set()
            for n, p in zip(names, self.params):
                st = optimizer.state[p]
                if len(st) == 0:   # same lazy init as torch.optim.Adam._init_group
                    st["step"] = torch.tensor(0.0, dtype=torch.float32)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                ptrs["m_" + n], ptrs["v_" + n] = ptr(st["exp_avg"]), ptr(st["exp_avg_sq"])
                self._state_refs.append((st["exp_avg"], st["exp_avg_sq"]))      # meta.c holds their raw addresses
                steps.add(int(float(st["step"])))
            assert len(steps) == 1, "parameters disagree on the Adam step count"
            b1, b2 = g["betas"]
            kw.update(lr=float(g["lr"]), beta1=float(b1), beta2=float(b2), eps=float(g["eps"]),
                      weight_decay=float(g["weight_decay"]), step=steps.pop())
        if need_grads:
            self.grads = [torch.zeros_like(p) for p in self.params]
            for n, gt in zip(names, self.grads):
                ptrs["g_" + n] = ptr(gt)
        # scratch for the forward pass's operand-ordered copy of W1 (sized for the larger, bf16x3 form)
        self.w1_image = torch.empty(max(lib().moc_w1_image_bytes(self.D, _lib.MOC_BF16),
                                        lib().moc_w1_image_bytes(self.D, _lib.MOC_F32)),
                                    dtype=torch.uint8, device=self.params[0].device)
        ptrs["W1_image"] = ptr(self.w1_image)
        self.c = MocMeta(**ptrs, **kw)

    # ---- one MetaState per (model, optimizer), reused from pass to pass: building the views costs 20-40 us of
    # Python, and the pass graphs (moc_train_steps_graph) are keyed on the tensors it points at
    _cache = weakref.WeakKeyDictionary()

    @classmethod
    def cached(cls, model, optimizer):
        ent = cls._cache.get(model)
        if ent is not None:
            meta, opt_ref, sig = ent
            if opt_ref() is optimizer and sig == cls._signature(meta.params, optimizer):
                meta.refresh()
                return meta
        meta = cls(model, optimizer)
        meta._graph_ok = True          # lives from pass to pass: worth capturing its passes
        cls._cache[model] = (meta, weakref.ref(optimizer), cls._signature(meta.params, optimizer))
        return meta

    @staticmethod
    def _signature(params, optimizer):
        sig = []
        for p in params:
            st = optimizer.state.get(p) or {}
            m, v = st.get("exp_avg"), st.get("exp_avg_sq")
            # storage addresses, not object identities: `.data = ` / `set_()` keep the id and move the storage, and the
            # fused kernels write through the raw pointers in meta.c
            sig.append((p.data_ptr(), m.data_ptr() if m is not None else 0, v.data_ptr() if v is not None else 0,
                        id(st.get("step"))))
        return tuple(sig)

    def refresh(self):
        """Hyper-parameters and step count as the optimizer holds them NOW (someone may have changed the learning
        rate, stepped it, or loaded a state dict in place)."""
        g = self._group
        b1, b2 = g["betas"]
        c = self.c
        c.lr, c.beta1, c.beta2, c.eps, c.weight_decay = float(g["lr"]), float(b1), float(b2), float(g["eps"]), float(g["weight_decay"])
        st = self.optimizer.state
        s0 = int(st[self.params[0]]["step"])
        assert all(int(st[p]["step"]) == s0 for p in self.params[1:]), "parameters disagree on the Adam step count"
        c.step = s0

    def step_graph(self):
        """The moc_step_graph_t of this meta-learner (created on first use).  None when switched off, and for a
        MetaState built for one call (not through `cached`): its graphs would be captured and thrown away."""
        if not (STEP_GRAPH and self._graph_ok):
            return None
        if self._graph is None:
            nbytes = lib().moc_step_graph_workspace_bytes(GRAPH_TABLE_STEPS)
            self._graph_ws = torch.empty(nbytes, dtype=torch.uint8, device=self.params[0].device)
            h = C.c_void_p()
            check(lib().moc_step_graph_create(ptr(self._graph_ws), nbytes, C.byref(h)), "moc_step_graph_create")
            self._graph = h
            weakref.finalize(self, lib().moc_step_graph_destroy, h).atexit = False   # (at exit the runtime goes first)
        return self._graph

    def graph_stats(self):
        """(captures, replays, passes that fell back to stream launches) of this meta-learner's pass graphs."""
        if self._graph is None:
            return (0, 0, 0)
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        check(lib().moc_step_graph_stats(self._graph, C.byref(a), C.byref(b), C.byref(c)), "moc_step_graph_stats")
        return a.value, b.value, c.value

    def advance(self, n_steps: int):
        """Record n fused Adam steps in the optimizer's own step counters."""
        self.c.step += n_steps
        for p in self.params:
            st = self.optimizer.state[p]["step"]
            st += n_steps   # tensor in-place (host or device scalar)


def draw_row_masks(total: int, out: torch.Tensor | None = None):
    """`total` keep flags from the CPU default generator, bit for bit what consecutive
    `torch.rand(n_i) > 0.5` calls (sum n_i == total) produce (main_moc.py:330), leaving the generator
    where they would.  Uses the library's mt19937 replay (several times faster than torch.rand);
    falls back to torch.rand itself when the generator state is not the layout it knows.
    Returns (uint8 host tensor [total], number of kept rows)."""
    if out is None:
        out = torch.empty(total, dtype=torch.uint8)
    if torch.get_default_dtype() == torch.float32:
        st = torch.get_rng_state()
        kept = lib().moc_host_draw_masks(ptr(st), st.numel(), total, ptr(out))
        if kept >= 0:
            torch.set_rng_state(st)
            return out, int(kept)
    m = torch.rand(total) > 0.5
    out.copy_(m)
    return out, int(m.sum())


def draw_row_masks_from(rng_state: torch.Tensor, total: int, out: torch.Tensor):
    """As draw_row_masks, but from the given generator state (a `torch.get_rng_state()` tensor), without
    touching torch's generator: -> (out, kept rows, state after the draws).  When the state's layout is not
    the one the library knows, torch itself draws from ITS generator and the third value is None."""
    if torch.get_default_dtype() == torch.float32:
        st = rng_state.clone()
        kept = lib().moc_host_draw_masks(ptr(st), st.numel(), total, ptr(out))
        if kept >= 0:
            return out, int(kept), st
    m = torch.rand(total) > 0.5
    out.copy_(m)
    return out, int(m.sum()), None


class MaskDrawer:
    """The keep flags of a pass, drawn one pass AHEAD on a helper thread (the reference has a DataLoader worker process
    beside its main thread; here the second host thread replays torch's mt19937: moc_host_draw_masks releases the GIL).

    The stream is sequential, so the flags of the pass after next follow from the generator state the last draw left:
    as soon as a draw for (state S, row layout L) is handed out, the draw for (S', L) starts in the background into a
    spare pinned buffer.  `take(S', L)` then returns it at once; any other request (someone else drew from the
    generator, another pass length) discards the speculation and draws in line -- the bits are always the ones
    `torch.rand(N) > 0.5` would give from the requested state.  Buffers are pinned host memory read in place by the
    compaction kernel: one is handed out again only after the event the caller attached to it has completed."""

    def __init__(self, total: int, row_off_c, n_slides: int, n_buffers: int = 4, pinned: bool = True):
        from concurrent.futures import ThreadPoolExecutor
        self.total, self.row_off_c, self.n_slides = int(total), row_off_c, int(n_slides)
        self.bufs = [torch.empty(self.total, dtype=torch.uint8) for _ in range(n_buffers)]
        if pinned:                                # (False: the CPU tests of the draw-ahead logic)
            self.bufs = [b.pin_memory() for b in self.bufs]
        self.busy = [None] * n_buffers            # event after the phase A that reads buffer i (None: free)
        self.pool = ThreadPoolExecutor(1)
        self.ahead = None                         # (state_before, buffer index, future)

    def _draw(self, state_before: torch.Tensor, i: int):
        st = state_before.clone()
        kept = lib().moc_host_draw_masks(ptr(st), st.numel(), self.total, ptr(self.bufs[i]))
        if kept < 0:
            return None
        mk = lib().moc_host_max_kept(self.bufs[i].data_ptr(), C.cast(self.row_off_c, C.c_void_p), self.n_slides)
        return int(kept), int(mk), st

    def _free_buffer(self, exclude=()):
        for i, ev in enumerate(self.busy):
            if i in exclude:
                continue
            if ev is None or ev.query():
                self.busy[i] = None
                return i
        for i, ev in enumerate(self.busy):        # none free: wait for the oldest the caller is done with
            if i not in exclude:
                ev.synchronize()
                self.busy[i] = None
                return i
        raise AssertionError("MaskDrawer: no buffer")

    def take(self, state_before: torch.Tensor, chain: bool = True):
        """-> (pinned flags, kept rows, max kept rows of a slide, generator state after, buffer index) or None when
        the generator state is not the layout the replay knows (the caller lets torch draw).  `chain` False: the pass
        after this one has another row layout (the caller starts ITS drawer): nothing is drawn ahead here."""
        if torch.get_default_dtype() != torch.float32:
            return None
        got = None
        if self.ahead is not None:
            st0, i, fut = self.ahead
            self.ahead = None
            res = fut.result()
            if res is not None and torch.equal(st0, state_before):
                got = (i, res)
            # (a discarded speculation leaves buffer i free: nothing on the GPU reads it)
        if got is None:
            i = self._free_buffer()
            res = self._draw(state_before, i)
            if res is None:
                return None
            got = (i, res)
        i, (kept, mk, st_after) = got
        if chain:                                 # the flags of the pass after this one, in the background
            j = self._free_buffer(exclude=(i,))
            self.ahead = (st_after, j, self.pool.submit(self._draw, st_after, j))
        return self.bufs[i], kept, mk, st_after, i

    def prefetch(self, state_before: torch.Tensor):
        """Start drawing the flags that follow `state_before` now (no-op when that is what is being drawn already):
        for a caller that learns early which pass comes next -- the draw then runs beside its kernel launches."""
        if torch.get_default_dtype() != torch.float32:
            return
        if self.ahead is not None:
            if torch.equal(self.ahead[0], state_before):
                return
            self.ahead[2].result()                # let the stale draw finish: its buffer is free again
            self.ahead = None
        j = self._free_buffer()
        self.ahead = (state_before.clone(), j, self.pool.submit(self._draw, state_before, j))

    def attach(self, i: int, event):
        """`event` completes when the GPU work that reads buffer i has run."""
        self.busy[i] = event


def train_use_bits(discard) -> int:
    return (~_lib.discard_bits(discard)) & 15            # main_moc.py:396-403


def eval_use_bits(discard) -> int:
    """main_moc.py:486-492: psi_p always; the last test is for "delta_bottomk"."""
    d = discard or ()
    return 1 | (0 if "delta_softmax" in d else 2) | (0 if "delta_diff" in d else 4) | (0 if "delta_bottomk" in d else 8)


def meta_forward(batch: SlideBatch, meta: MetaState, slide0: int, n: int, use_bits: int, keep_hidden: bool = True):
    """keep_hidden=False (evaluation): H1 and the gates are not written -- only the backward pass reads them."""
    _, ws = batch.meta_ws()
    if not keep_hidden:
        ws = type(ws).from_buffer_copy(ws)
        ws.H1 = None
        ws.gates = None
    check(lib().moc_meta_forward(C.byref(batch.c), C.byref(meta.c), C.byref(ws), slide0, n, use_bits, _stream()),
          "moc_meta_forward")


def meta_forward_dense(batch: SlideBatch, meta: MetaState, slide0: int, n: int, use_bits: int,
                       gates: torch.Tensor | None, mixed: torch.Tensor):
    """Patch maps: the gates [total, 4] (nullable) and mixed scores [C, total] of EVERY row of slides slide0 .. +n of an
    unmasked batch whose score pass has run, into the caller's tensors -- at a selected row the bits meta_forward gives it
    (moc_meta_forward_dense)."""
    T = batch.total
    assert batch.mask is None, "meta_forward_dense: the batch must be unmasked"
    assert mixed.is_cuda and mixed.dtype == torch.float32 and mixed.is_contiguous() and tuple(mixed.shape) == (batch.C, T)
    if gates is not None:
        assert gates.is_cuda and gates.dtype == torch.float32 and gates.is_contiguous() and tuple(gates.shape) == (T, 4)
    check(lib().moc_meta_forward_dense(C.byref(batch.c), C.byref(meta.c), ptr(gates), ptr(mixed), slide0, n, use_bits,
                                       _stream()), "moc_meta_forward_dense")


class ModelArena:
    """R senet state_dicts (`model.<i>.weight` / `.bias` of senet(D, 4)) packed the way moc_meta_forward_models reads them:
    model r's W1 | b1 | W2 | b2 at row r of one [R, par_stride] fp32 arena, its W1 operand image at row r of an
    [R, image_stride] byte arena (the entry rebuilds the images).  `c`: the moc_meta_t of model 0, `runs`: the moc_runs_t."""

    KEYS = ("model.0.weight", "model.0.bias", "model.2.weight", "model.2.bias")
    MAX_MODELS = 64          # of_models (an entry point takes sixteen of them per call: `group`)

    @staticmethod
    def layout(D):
        """(offsets of W1 | b1 | W2 | b2 inside a model's block, floats of one model, shapes)."""
        offs = (0, HIDDEN * D, HIDDEN * D + HIDDEN, HIDDEN * D + HIDDEN + 4 * HIDDEN)
        return offs, offs[3] + 4, ((HIDDEN, D), (HIDDEN,), (4, HIDDEN), (4,))

    def __init__(self, state_dicts, device):
        R = len(state_dicts)
        assert 1 <= R <= 16, "ModelArena: 1 .. 16 models"
        self._copy(state_dicts, device)

    def _seat(self, base, R, D, par_stride, device):
        """The object over R models whose blocks start `par_stride` floats apart from address `base` on: the operand-image
        scratch, `c` (model 0's moc_meta_t) and `runs` (the first sixteen models at most; `group` for the others)."""
        offs, _, _ = self.layout(D)
        self.R, self.D, self.device, self.par_stride = R, D, device, int(par_stride)
        img_b = max(lib().moc_w1_image_bytes(D, _lib.MOC_BF16), lib().moc_w1_image_bytes(D, _lib.MOC_F32))
        self.img_stride = (img_b + 255) // 256 * 256
        self.images = torch.empty((R, self.img_stride), dtype=torch.uint8, device=device)
        self.c = MocMeta(W1=base, b1=base + 4 * offs[1], W2=base + 4 * offs[2], b2=base + 4 * offs[3],
                         W1_image=ptr(self.images), H=HIDDEN, D=D)
        self.runs = MocRuns(n_runs=min(R, 16), slide_stride=0, par_stride=self.par_stride, image_stride=self.img_stride)

    def _copy(self, state_dicts, device):
        """A scratch arena `P` [R, par_stride] holding copies of the state dicts' tensors."""
        R = len(state_dicts)
        D = int(state_dicts[0]["model.0.weight"].shape[1])
        offs, n_par, shapes = self.layout(D)
        for sd in state_dicts:
            assert all(tuple(sd[k].shape) == s for k, s in zip(self.KEYS, shapes)), f"ModelArena: every model must be senet({D}, 4)"
        self.P = torch.zeros((R, (n_par + 63) // 64 * 64), dtype=torch.float32, device=device)
        for r, sd in enumerate(state_dicts):
            for k, o in zip(self.KEYS, offs):
                t = sd[k].detach().reshape(-1)
                self.P[r, o:o + t.numel()].copy_(t.to(device=device, dtype=torch.float32))
        self._seat(ptr(self.P), R, D, self.P.size(1), device)

    @classmethod
    def of_models(cls, models):
        """The arena of R live senets (any R up to MAX_MODELS), for the evaluation of several runs in one pass
        (meta_forward_by_slide).  Where the models' parameter tensors already lie in one arena -- after runs.TrainRuns they
        are views of TrainRuns.P, W1 | b1 | W2 | b2 of a run in one block, the runs a constant stride apart -- the arena is
        used IN PLACE: no copy, `P` is None (the storage is the models' own, kept alive through `_keep`), only the operand
        images are scratch of this object; `c`, `runs` and `group` are as for a copied arena, so every entry that takes a
        ModelArena takes this one.  Otherwise the parameters are copied into a scratch arena.  Either way the values are
        those of the models at the time of the call."""
        R = len(models)
        assert 1 <= R <= cls.MAX_MODELS, f"ModelArena.of_models: 1 .. {cls.MAX_MODELS} models"
        quads = [[m.model[0].weight, m.model[0].bias, m.model[2].weight, m.model[2].bias] for m in models]
        D = int(quads[0][0].shape[1])
        offs, n_par, shapes = cls.layout(D)
        assert all(tuple(p.shape) == sh for q in quads for p, sh in zip(q, shapes)), \
            f"evaluation of several runs: every model must be senet({D}, 4) (models of different width are not batched)"
        dev = quads[0][0].device
        ok = all(p.is_cuda and p.device == dev and p.dtype == torch.float32 and p.data.is_contiguous() for q in quads for p in q)
        base = quads[0][0].data_ptr()
        step = (quads[1][0].data_ptr() - base) if R > 1 else 4 * n_par
        ok = ok and step % 4 == 0 and step >= 4 * n_par
        ok = ok and all(p.data_ptr() == base + r * step + 4 * o for r, q in enumerate(quads) for p, o in zip(q, offs))
        self = cls.__new__(cls)
        if ok:
            self.P, self._keep = None, quads
            self._seat(base, R, D, step // 4, dev)
        else:
            self._copy([{k: p.detach() for k, p in zip(cls.KEYS, q)} for q in quads], dev)
        return self

    def group(self, r0: int, n_models: int):
        """(moc_meta_t, moc_runs_t) of models r0 .. r0 + n_models - 1 (at most sixteen: what one call serves)."""
        assert 0 <= r0 and 1 <= n_models <= 16 and r0 + n_models <= self.R
        mc = MocMeta.from_buffer_copy(self.c)
        for name in ("W1", "b1", "W2", "b2"):
            setattr(mc, name, getattr(self.c, name) + 4 * r0 * self.par_stride)
        mc.W1_image = ptr(self.images) + r0 * self.img_stride
        return mc, MocRuns(n_runs=n_models, slide_stride=0, par_stride=self.par_stride, image_stride=self.img_stride)


def meta_forward_models(batch: SlideBatch, params: ModelArena, n_models: int, mixed: torch.Tensor, slide0: int, n: int,
                        use_bits: int):
    """The evaluation forward of n_models meta-learners (the first n_models of `params`) over the union rows of slides
    slide0 .. +n of an unmasked batch whose phase A has run, in one launch: mixed [n_models, C, total] -- slab r is what
    meta_forward gives with model r alone (moc_meta_forward_models)."""
    T = batch.total
    assert batch.mask is None, "meta_forward_models: the batch must be unmasked"
    assert 1 <= n_models <= params.R and params.D == batch.D, "meta_forward_models: models / width do not match"
    assert mixed.is_cuda and mixed.dtype == torch.float32 and mixed.is_contiguous() and \
        tuple(mixed.shape) == (n_models, batch.C, T)
    runs = MocRuns.from_buffer_copy(params.runs)
    runs.n_runs = n_models
    check(lib().moc_meta_forward_models(C.byref(batch.c), C.byref(params.c), C.byref(runs), ptr(mixed), slide0, n, use_bits,
                                        _stream()), "moc_meta_forward_models")


def meta_forward_by_slide(batch: SlideBatch, params: ModelArena, r0: int, n_models: int, model_of_slide: torch.Tensor,
                          slide0: int, n: int, use_bits: int, keep_hidden: bool = False):
    """The evaluation forward over the union rows of slides slide0 .. +n of an unmasked batch whose phase A has run, in one
    launch, every slide with a model of its own: slide b of the batch is scored by model r0 + model_of_slide[b] of `params`
    (device int32 [batch.n_slides], values 0 .. n_models - 1, n_models <= 16).  Writes the batch's own `mixed` as meta_forward
    does -- for a slide of model r the bits meta_forward gives with model r alone -- so that one pool_loss pools all slides
    (moc_meta_forward_by_slide)."""
    assert batch.mask is None, "meta_forward_by_slide: the batch must be unmasked"
    assert params.D == batch.D, "meta_forward_by_slide: models / width do not match"
    assert model_of_slide.is_cuda and model_of_slide.dtype == torch.int32 and model_of_slide.is_contiguous() and \
        model_of_slide.numel() == batch.n_slides, "meta_forward_by_slide: model_of_slide is device int32 [n_slides]"
    assert not (keep_hidden and getattr(batch, "eval_only", False)), "meta_forward_by_slide: this batch keeps no H1 / gates"
    mc, runs = params.group(r0, n_models)
    _, ws = batch.meta_ws()
    if not keep_hidden:
        ws = type(ws).from_buffer_copy(ws)
        ws.H1 = None
        ws.gates = None
    check(lib().moc_meta_forward_by_slide(C.byref(batch.c), C.byref(mc), C.byref(runs), ptr(model_of_slide), C.byref(ws),
                                          slide0, n, use_bits, _stream()), "moc_meta_forward_by_slide")


def meta_forward_dense_models(batch: SlideBatch, params: ModelArena, n_models: int, scale: float, prob_mean: torch.Tensor,
                              prob_std: torch.Tensor | None, gates_mean: torch.Tensor | None, slide0: int, n: int,
                              use_bits: int):
    """Ensemble patch maps: the dense forward of n_models meta-learners (the first n_models of `params`) over EVERY row of
    slides slide0 .. +n of an unmasked batch whose score pass has run, reduced over the models on the device --
    prob_mean / prob_std [C, total]: mean and population std of softmax(scale * mixed_r); gates_mean [total, 4]: the mean
    gates (moc_meta_forward_dense_models).  prob_std and gates_mean may be None."""
    T = batch.total
    assert batch.mask is None, "meta_forward_dense_models: the batch must be unmasked"
    assert 1 <= n_models <= params.R and params.D == batch.D, "meta_forward_dense_models: models / width do not match"
    assert prob_mean is not None, "meta_forward_dense_models: prob_mean is required"
    for t, shape in ((prob_mean, (batch.C, T)), (prob_std, (batch.C, T)), (gates_mean, (T, 4))):
        if t is not None:
            assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == shape
    runs = MocRuns.from_buffer_copy(params.runs)
    runs.n_runs = n_models
    check(lib().moc_meta_forward_dense_models(C.byref(batch.c), C.byref(params.c), C.byref(runs), float(scale),
                                              ptr(prob_mean), ptr(prob_std), ptr(gates_mean), slide0, n, use_bits,
                                              _stream()), "moc_meta_forward_dense_models")


def pool_models(batch: SlideBatch, mixed: torch.Tensor, labels: torch.Tensor, slide0: int, n: int):
    """moc_pool_loss over every model's slab of `mixed` [R, C, total] -> dict of per-model pooled [R, n_slides, C], pred,
    loss [R, n_slides] and topk_idx / topk_cnt (labels: device int64 [n_slides]; zeros for unlabeled slides -- the loss
    is then meaningless)."""
    t, ws = batch.meta_ws()
    R, ns, Cc, K = mixed.size(0), batch.n_slides, batch.C, batch.topk
    dev = mixed.device
    out = dict(pooled=torch.empty((R, ns, Cc), dtype=torch.float32, device=dev),
               topk_idx=torch.empty((R, ns, Cc, K), dtype=torch.int32, device=dev),
               topk_cnt=torch.empty((R, ns, Cc), dtype=torch.int32, device=dev),
               loss=torch.empty((R, ns), dtype=torch.float32, device=dev),
               pred=torch.empty((R, ns), dtype=torch.int32, device=dev))
    for r in range(R):
        w = type(ws).from_buffer_copy(ws)
        w.mixed = ptr(mixed[r])
        for k in ("pooled", "topk_idx", "topk_cnt", "loss", "pred"):
            setattr(w, k, ptr(out[k][r]))
        check(lib().moc_pool_loss(C.byref(batch.c), C.byref(w), ptr(labels), slide0, n, _stream()), "moc_pool_loss")
    return out


def mix_fixed(batch: SlideBatch, slide0: int, n: int, mode: str):
    _, ws = batch.meta_ws()
    code = {"avg": 0, "sum": 1, "max": 2}[mode]
    check(lib().moc_mix_fixed(C.byref(batch.c), C.byref(ws), slide0, n, code, _stream()), "moc_mix_fixed")


def pool_loss(batch: SlideBatch, labels: torch.Tensor, slide0: int, n: int):
    _, ws = batch.meta_ws()
    check(lib().moc_pool_loss(C.byref(batch.c), C.byref(ws), ptr(labels), slide0, n, _stream()), "moc_pool_loss")


def loss_only(batch: SlideBatch, labels: torch.Tensor, slide0: int, n: int):
    """CE + argmax of ws.pooled[slide0:slide0+n] (already filled) into ws.loss / ws.pred."""
    t, _ = batch.meta_ws()
    check(lib().moc_ce_loss(ptr(t["pooled"][slide0:]), ptr(labels[slide0:]), n, batch.C,
                            ptr(t["loss"][slide0:]), ptr(t["pred"][slide0:]), _stream()), "moc_ce_loss")


def ce_loss(pooled: torch.Tensor, labels: torch.Tensor):
    """(loss [n] float32, pred [n] int32): CE + argmax of the rows of `pooled` [n, C] (float32, contiguous)."""
    n, Cc = pooled.shape
    loss = torch.empty(n, dtype=torch.float32, device=pooled.device)
    pred = torch.empty(n, dtype=torch.int32, device=pooled.device)
    check(lib().moc_ce_loss(ptr(pooled), ptr(labels), n, Cc, ptr(loss), ptr(pred), _stream()), "moc_ce_loss")
    return loss, pred


def train_steps(batch: SlideBatch, meta: MetaState, labels: torch.Tensor, slide0: int, n: int, use_bits: int):
    """n consecutive meta-steps (one slide each) with Adam applied in place: one graph launch per pass when the
    meta-learner has a step graph (MOC_STEP_GRAPH=1, opt-in), 2 n + 1 stream launches otherwise -- same kernels,
    same coefficient floats, bit-identical parameters."""
    _, ws = batch.meta_ws()
    g = meta.step_graph()
    # (a pass graph bakes its grids in: the device's n_sel there)
    batch.publish_n_sel(allow=g is None)
    if g is not None:
        check(lib().moc_train_steps_graph(g, C.byref(batch.c), C.byref(meta.c), C.byref(ws), ptr(labels), slide0, n,
                                          use_bits, _stream()), "moc_train_steps_graph")
    else:
        check(lib().moc_train_steps(C.byref(batch.c), C.byref(meta.c), C.byref(ws), ptr(labels), slide0, n,
                                    use_bits, _stream()), "moc_train_steps")
    meta.advance(n)


def train_steps_dp(batch: SlideBatch, meta: MetaState, labels: torch.Tensor, slide0: int, n: int, use_bits: int,
                   grad_flat: torch.Tensor, allreduce_fn, comm, world: int):
    """n synchronous data-parallel steps on this rank's slides; `allreduce_fn` is the address of a
    function with ncclAllReduce's signature (None at world 1).  Does not advance the step counters."""
    _, ws = batch.meta_ws()
    check(lib().moc_train_steps_dp(C.byref(batch.c), C.byref(meta.c), C.byref(ws), ptr(labels), slide0, n,
                                   use_bits, ptr(grad_flat), grad_flat.numel(), allreduce_fn, comm, world,
                                   _stream()), "moc_train_steps_dp")


def fused_step_shape(batch: SlideBatch) -> bool:
    """Whether the node-local exchange step applies -- decided from C, topk, D, topj only."""
    c = batch.c
    return bool(lib().moc_p2p_step_supported(c.C, c.topk, c.D, c.topj))


def train_steps_p2p(batch: SlideBatch, meta: MetaState, labels: torch.Tensor, slide0: int, n: int, use_bits: int,
                    comm_handle):
    """n synchronous data-parallel steps with the gradient exchange inside the step kernel
    (moc_p2p_*: peer-mapped receive buffers on one node).  Does not advance the step counters."""
    _, ws = batch.meta_ws()
    check(lib().moc_train_steps_p2p(C.byref(batch.c), C.byref(meta.c), C.byref(ws), ptr(labels), slide0, n,
                                    use_bits, comm_handle, _stream()), "moc_train_steps_p2p")


def train_grad(batch: SlideBatch, meta: MetaState, labels: torch.Tensor, slide: int, use_bits: int):
    """Forward + loss + gradients of one slide into meta.grads (no update)."""
    _, ws = batch.meta_ws()
    check(lib().moc_train_grad(C.byref(batch.c), C.byref(meta.c), C.byref(ws), ptr(labels), slide, use_bits,
                               _stream()), "moc_train_grad")


def adam_step(meta: MetaState, grad_scale: float = 1.0, advance: bool = True):
    check(lib().moc_adam_step(C.byref(meta.c), C.c_float(grad_scale), _stream()), "moc_adam_step")
    if advance:
        meta.advance(1)


def topk_mean(keys: torch.Tensor, vals: torch.Tensor, K: int, smallest=False, key_shared=False,
              want_idx=False, seg_off: torch.Tensor | None = None):
    """keys/vals: [C, N] device fp32 (keys may be [1, N] with key_shared).  Returns
    pooled [n_seg, C] (and idx [n_seg, C, K], cnt [n_seg, C])."""
    assert keys.is_cuda and vals.is_cuda and keys.dtype == vals.dtype == torch.float32
    keys, vals = keys.contiguous(), vals.contiguous()
    Cc, N = vals.shape
    dev = vals.device
    if seg_off is None:
        seg_off = torch.tensor([0, N], dtype=torch.int64, device=dev)
    n_seg = seg_off.numel() - 1
    pooled = torch.empty((n_seg, Cc), dtype=torch.float32, device=dev)
    idx = torch.empty((n_seg, Cc, K), dtype=torch.int32, device=dev) if want_idx else None
    cnt = torch.empty((n_seg, Cc), dtype=torch.int32, device=dev) if want_idx else None
    check(lib().moc_topk_mean(ptr(keys), 0 if key_shared else N, ptr(vals), N, ptr(seg_off), None, n_seg, Cc,
                              int(K), int(bool(smallest)), ptr(pooled), ptr(idx), ptr(cnt), _stream()),
          "moc_topk_mean")
    return (pooled, idx, cnt) if want_idx else pooled


MULTI_MAX_K, MULTI_MAX_NK = 64, 8       # moc_topk_mean_multi: one rank per lane; the Ks travel in the kernel's arguments


def topk_mean_multi(keys: torch.Tensor, vals: torch.Tensor, Ks, smallest=False, key_shared=False,
                    want_idx=False, seg_off: torch.Tensor | None = None, seg_len: torch.Tensor | None = None):
    """topk_mean at every K of `Ks` (at most 8, each at most 64) from ONE ranking: pooled [n_K, n_seg, C], slab i bit for
    bit topk_mean(..., Ks[i]) (and, with want_idx, idx [n_seg, C, max(Ks)], cnt [n_seg, C] as topk_mean at max(Ks)).
    seg_len (device int32 [n_seg], optional): segment lengths where they are not the gaps of seg_off."""
    assert keys.is_cuda and vals.is_cuda and keys.dtype == vals.dtype == torch.float32
    Ks = [int(k) for k in Ks]
    keys, vals = keys.contiguous(), vals.contiguous()
    Cc, N = vals.shape
    dev = vals.device
    if seg_off is None:
        seg_off = torch.tensor([0, N], dtype=torch.int64, device=dev)
    n_seg = seg_len.numel() if seg_len is not None else seg_off.numel() - 1
    pooled = torch.empty((len(Ks), n_seg, Cc), dtype=torch.float32, device=dev)
    kmax = max(Ks) if Ks else 1
    idx = torch.empty((n_seg, Cc, kmax), dtype=torch.int32, device=dev) if want_idx else None
    cnt = torch.empty((n_seg, Cc), dtype=torch.int32, device=dev) if want_idx else None
    ks_c = (C.c_int32 * max(len(Ks), 1))(*Ks)
    check(lib().moc_topk_mean_multi(ptr(keys), 0 if key_shared else N, ptr(vals), N, ptr(seg_off), ptr(seg_len), n_seg, Cc,
                                    C.cast(ks_c, C.c_void_p), len(Ks), int(bool(smallest)), ptr(pooled), ptr(idx), ptr(cnt),
                                    _stream()), "moc_topk_mean_multi")
    return (pooled, idx, cnt) if want_idx else pooled


def gated_attention_pool(h: torch.Tensor, Wa, ba, Wb, bb, Wc, bc):
    """SURVEY.md section 8 row f4 (models/model_clam.py:41-64, :178-183, :206): h [N, L] fp32 on the GPU,
    Wa / Wb [D, L], Wc [K, D] in nn.Linear layout.  -> (A_raw [K, N], M [K, L])."""
    ts = [h, Wa, ba, Wb, bb, Wc, bc]
    assert all(t.is_cuda and t.dtype == torch.float32 for t in ts), "gated_attention_pool: fp32 tensors on the GPU"
    h, Wa, ba, Wb, bb, Wc, bc = [t.detach().contiguous() for t in ts]
    N, L = h.shape
    D, K = Wa.shape[0], Wc.shape[0]
    assert Wa.shape == Wb.shape == (D, L) and Wc.shape == (K, D) and ba.numel() == bb.numel() == D and bc.numel() == K
    dev = h.device
    A_raw = torch.empty((K, N), dtype=torch.float32, device=dev)
    M = torch.empty((K, L), dtype=torch.float32, device=dev)
    nbytes = lib().moc_gated_attention_workspace(N, L, D, K)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
    check(lib().moc_gated_attention_pool(ptr(h), N, L, ptr(Wa), ptr(ba), ptr(Wb), ptr(bb), D, ptr(Wc), ptr(bc), K,
                                         ptr(A_raw), ptr(M), ptr(ws), nbytes, _stream()), "moc_gated_attention_pool")
    return A_raw, M


def gated_attention_backward(h, Wa, ba, Wb, bb, Wc, A_raw, gA=None, gM=None):
    """The backward of gated_attention_pool (include/moc_hip.h moc_gated_attention_backward; autograd's work behind
    models/model_clam.py:58-63, :178-183, :206).  One recompute pass in HIP, then two plain GEMMs as library calls.
    -> (dh [N, L], dWa [D, L], dba [D], dWb [D, L], dbb [D], dWc [K, D], dbc [K])."""
    ts = [h, Wa, ba, Wb, bb, Wc, A_raw] + [g for g in (gA, gM) if g is not None]
    assert all(t.is_cuda and t.dtype == torch.float32 for t in ts), "gated_attention_backward: fp32 tensors on the GPU"
    h, Wa, ba, Wb, bb, Wc, A_raw = [t.detach().contiguous() for t in (h, Wa, ba, Wb, bb, Wc, A_raw)]
    gA = gA.detach().contiguous() if gA is not None else None
    gM = gM.detach().contiguous() if gM is not None else None
    N, L = h.shape
    D, K = Wa.shape[0], Wc.shape[0]
    assert Wa.shape == Wb.shape == (D, L) and Wc.shape == (K, D) and A_raw.shape == (K, N)
    assert (gA is None or gA.shape == (K, N)) and (gM is None or gM.shape == (K, L))
    dev = h.device
    S = lib().moc_gated_attention_dab_stride(D, K)
    dab = torch.empty((N, S), dtype=torch.float32, device=dev)     # da | db | p | 0
    ds = torch.empty((K, N), dtype=torch.float32, device=dev)
    dcol = torch.empty(((2 + K) * D,), dtype=torch.float32, device=dev)
    dbc = torch.empty((K,), dtype=torch.float32, device=dev)
    nbytes = lib().moc_gated_attention_backward_workspace(N, L, D, K)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
    check(lib().moc_gated_attention_backward(ptr(h), N, L, ptr(Wa), ptr(ba), ptr(Wb), ptr(bb), D, ptr(Wc), K, ptr(A_raw),
                                             ptr(gA) if gA is not None else None, ptr(gM) if gM is not None else None,
                                             ptr(dab), ptr(ds), ptr(dcol), ptr(dbc), ptr(ws), nbytes, _stream()),
          "moc_gated_attention_backward")
    X = torch.zeros((S, L), dtype=torch.float32, device=dev)       # [Wa; Wb; gM; 0]: M = p h rides in the same GEMM
    X[:D], X[D:2 * D] = Wa, Wb
    if gM is not None:
        X[2 * D:2 * D + K] = gM
    dh = dab @ X
    dW = dab.t() @ h                                               # [S, L]: dWa over dWb (over M)
    return dh, dW[:D], dcol[:D], dW[D:2 * D], dcol[D:2 * D], dcol[2 * D:].view(K, D), dbc


ADAPTER_C, ADAPTER_H, ADAPTER_MAX_E, ADAPTER_MAX_CLASSES = 512, 128, 8, 64      # what moc_adapter_logits is built for


def adapter_logits(feat: torch.Tensor, W1s, W2s, router, classifier: torch.Tensor, ratio: float) -> torch.Tensor:
    """SURVEY.md section 8 row f3 (models/model_adapters.py:185-193, :330-405 with the soft router): the per-patch logits
    [N, C] of a CLIP-Adapter (one (W1, W2) pair, router None) or a MoE-adapter bag (E pairs, router [E, c]) in one pass
    over feat [N, 512] (include/moc_hip.h moc_adapter_logits).  W1s[e] [128, 512], W2s[e] [512, 128] (nn.Linear layout),
    classifier [512, C]; `ratio` is the mixing weight the module stores (clip_ratio, or clip_ratio / E).  No gradient."""
    W1s, W2s = list(W1s), list(W2s)
    ts = [feat, classifier] + W1s + W2s + ([router] if router is not None else [])
    assert all(t.is_cuda and t.dtype == torch.float32 for t in ts), "adapter_logits: fp32 tensors on the GPU (no CPU fallback)"
    assert len(W1s) == len(W2s) >= 1 and (router is None) == (len(W1s) == 1), "adapter_logits: one router row per expert, none for one"
    feat, classifier = feat.detach().contiguous(), classifier.detach().contiguous()
    W1s, W2s = [w.detach().contiguous() for w in W1s], [w.detach().contiguous() for w in W2s]
    router = router.detach().contiguous() if router is not None else None
    N, c = feat.shape
    E, h, Cc = len(W1s), W1s[0].shape[0], classifier.shape[1]
    assert all(w.shape == (h, c) for w in W1s) and all(w.shape == (c, h) for w in W2s) and classifier.shape[0] == c
    assert router is None or router.shape == (E, c)
    dev = feat.device
    logits = torch.empty((N, Cc), dtype=torch.float32, device=dev)
    nbytes = lib().moc_adapter_workspace(N, c, h, E, Cc)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
    p1, p2 = (C.c_void_p * E)(*[w.data_ptr() for w in W1s]), (C.c_void_p * E)(*[w.data_ptr() for w in W2s])
    check(lib().moc_adapter_logits(ptr(feat), N, c, C.cast(p1, C.c_void_p), C.cast(p2, C.c_void_p), h, E, ptr(router),
                                   ptr(classifier), Cc, C.c_float(float(ratio)), ptr(logits), ptr(ws), nbytes, _stream()),
          "moc_adapter_logits")
    return logits


NYSTROM_HEADS, NYSTROM_DIM_HEAD, NYSTROM_LANDMARKS, NYSTROM_MAX_TAPS = 8, 64, 256, 33   # what moc_nystrom_* is built for


def _nystrom_qkv(qkv: torch.Tensor, what: str) -> int:
    assert qkv.is_cuda and qkv.dtype == torch.float32, f"{what}: fp32 tensors on the GPU (no CPU fallback)"
    assert qkv.dim() == 2 and qkv.shape[1] == 3 * NYSTROM_HEADS * NYSTROM_DIM_HEAD and qkv.is_contiguous(), \
        f"{what}: qkv must be a contiguous [n_pad, 1536]"
    n_pad = qkv.shape[0]
    assert n_pad >= NYSTROM_LANDMARKS and n_pad % NYSTROM_LANDMARKS == 0, f"{what}: n_pad={n_pad} is no multiple of 256"
    return n_pad


def _nystrom_hmd(t: torch.Tensor, name: str, what: str) -> torch.Tensor:
    assert t.is_cuda and t.dtype == torch.float32, f"{what}: fp32 tensors on the GPU (no CPU fallback)"
    assert t.shape == (NYSTROM_HEADS, NYSTROM_LANDMARKS, NYSTROM_DIM_HEAD), f"{what}: {name} must be [8, 256, 64]"
    return t.detach().contiguous()


def nystrom_landmark_values(qkv: torch.Tensor, q_l: torch.Tensor) -> torch.Tensor:
    """Kernel A of the fused Nystrom forward (include/moc_hip.h moc_nystrom_landmark_values): W [8, 256, 64], for each
    head softmax_over_tokens(q_l k^T) v, from qkv [n_pad, 1536] as to_qkv leaves it and the scaled landmark queries q_l
    [8, 256, 64].  No score matrix is formed; no gradient."""
    what = "nystrom_landmark_values"
    n_pad = _nystrom_qkv(qkv, what)
    q_l = _nystrom_hmd(q_l, "q_l", what)
    W = torch.empty_like(q_l)
    nbytes = lib().moc_nystrom_workspace(n_pad, NYSTROM_HEADS, NYSTROM_DIM_HEAD, NYSTROM_LANDMARKS)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=qkv.device)
    check(lib().moc_nystrom_landmark_values(ptr(qkv.detach()), n_pad, NYSTROM_HEADS, NYSTROM_DIM_HEAD, NYSTROM_LANDMARKS,
                                            ptr(q_l), ptr(W), ptr(ws), nbytes, _stream()), "moc_nystrom_landmark_values")
    return W


def nystrom_token_values(qkv: torch.Tensor, k_l: torch.Tensor, Y: torch.Tensor, conv_w, scale: float) -> torch.Tensor:
    """Kernel B of the fused Nystrom forward (moc_nystrom_token_values): out [n_pad, 512], token-major, for each token
    and head softmax_256(scale q k_l^T) Y + the depth-wise residual convolution of v with conv_w [8, taps] (None: no
    residual).  k_l, Y: [8, 256, 64].  No gradient."""
    what = "nystrom_token_values"
    n_pad = _nystrom_qkv(qkv, what)
    k_l, Y = _nystrom_hmd(k_l, "k_l", what), _nystrom_hmd(Y, "Y", what)
    taps = 0
    if conv_w is not None:
        assert conv_w.is_cuda and conv_w.dtype == torch.float32, f"{what}: fp32 tensors on the GPU (no CPU fallback)"
        assert conv_w.dim() == 2 and conv_w.shape[0] == NYSTROM_HEADS, f"{what}: conv_w must be [8, taps]"
        taps = conv_w.shape[1]
        assert taps % 2 == 1 and taps <= NYSTROM_MAX_TAPS, f"{what}: taps={taps} must be odd and at most 33"
        conv_w = conv_w.detach().contiguous()
    out = torch.empty((n_pad, NYSTROM_HEADS * NYSTROM_DIM_HEAD), dtype=torch.float32, device=qkv.device)
    check(lib().moc_nystrom_token_values(ptr(qkv.detach()), n_pad, NYSTROM_HEADS, NYSTROM_DIM_HEAD, NYSTROM_LANDMARKS, ptr(k_l),
                                         ptr(Y), ptr(conv_w), taps, C.c_float(float(scale)), ptr(out), _stream()),
          "moc_nystrom_token_values")
    return out


def nystrom_landmark_values_lse(qkv: torch.Tensor, q_l: torch.Tensor):
    """nystrom_landmark_values that also returns the per-landmark log-sum-exp over the tokens, [8, 256], from which the
    backward recomputes the weights (moc_nystrom_landmark_values_lse): (W, lse), W bit for bit the other entry's."""
    what = "nystrom_landmark_values_lse"
    n_pad = _nystrom_qkv(qkv, what)
    q_l = _nystrom_hmd(q_l, "q_l", what)
    W = torch.empty_like(q_l)
    lse = torch.empty((NYSTROM_HEADS, NYSTROM_LANDMARKS), dtype=torch.float32, device=qkv.device)
    nbytes = lib().moc_nystrom_workspace(n_pad, NYSTROM_HEADS, NYSTROM_DIM_HEAD, NYSTROM_LANDMARKS)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=qkv.device)
    check(lib().moc_nystrom_landmark_values_lse(ptr(qkv.detach()), n_pad, NYSTROM_HEADS, NYSTROM_DIM_HEAD, NYSTROM_LANDMARKS,
                                                ptr(q_l), ptr(W), ptr(lse), ptr(ws), nbytes, _stream()),
          "moc_nystrom_landmark_values_lse")
    return W, lse


def _nystrom_backward_ws(n_pad: int, device):
    nbytes = lib().moc_nystrom_backward_workspace(n_pad, NYSTROM_HEADS, NYSTROM_DIM_HEAD, NYSTROM_LANDMARKS)
    return torch.empty(max(nbytes, 16), dtype=torch.uint8, device=device), nbytes


def nystrom_landmark_backward(qkv: torch.Tensor, q_l: torch.Tensor, W: torch.Tensor, lse: torch.Tensor, dW: torch.Tensor):
    """Backward of nystrom_landmark_values_lse (moc_nystrom_landmark_backward): (dqkv [n_pad, 1536], dq_l [8, 256, 64]) from
    its inputs, its two results and dW [8, 256, 64].  dqkv holds dk and dv and exact zeros in the q columns.  The weights are
    recomputed from lse; no score matrix is formed."""
    what = "nystrom_landmark_backward"
    n_pad = _nystrom_qkv(qkv, what)
    q_l, W, dW = _nystrom_hmd(q_l, "q_l", what), _nystrom_hmd(W, "W", what), _nystrom_hmd(dW, "dW", what)
    assert lse.is_cuda and lse.dtype == torch.float32, f"{what}: fp32 tensors on the GPU (no CPU fallback)"
    assert lse.shape == (NYSTROM_HEADS, NYSTROM_LANDMARKS), f"{what}: lse must be [8, 256]"
    lse = lse.detach().contiguous()
    dqkv, dq_l = torch.empty_like(qkv, requires_grad=False), torch.empty_like(q_l)
    ws, nbytes = _nystrom_backward_ws(n_pad, qkv.device)
    check(lib().moc_nystrom_landmark_backward(ptr(qkv.detach()), n_pad, NYSTROM_HEADS, NYSTROM_DIM_HEAD, NYSTROM_LANDMARKS,
                                              ptr(q_l), ptr(W), ptr(lse), ptr(dW), ptr(dqkv), ptr(dq_l), ptr(ws), nbytes,
                                              _stream()), "moc_nystrom_landmark_backward")
    return dqkv, dq_l


def nystrom_token_backward(qkv: torch.Tensor, k_l: torch.Tensor, Y: torch.Tensor, scale: float, dout: torch.Tensor):
    """Backward of nystrom_token_values without a residual (moc_nystrom_token_backward): (dqkv [n_pad, 1536], dk_l, dY
    [8, 256, 64]) from its inputs and dout [n_pad, 512].  dqkv holds dq and exact zeros in the k and v columns."""
    what = "nystrom_token_backward"
    n_pad = _nystrom_qkv(qkv, what)
    k_l, Y = _nystrom_hmd(k_l, "k_l", what), _nystrom_hmd(Y, "Y", what)
    assert dout.is_cuda and dout.dtype == torch.float32, f"{what}: fp32 tensors on the GPU (no CPU fallback)"
    assert dout.shape == (n_pad, NYSTROM_HEADS * NYSTROM_DIM_HEAD), f"{what}: dout must be [n_pad, 512]"
    dout = dout.detach().contiguous()
    dqkv, dk_l, dY = torch.empty_like(qkv, requires_grad=False), torch.empty_like(k_l), torch.empty_like(Y)
    ws, nbytes = _nystrom_backward_ws(n_pad, qkv.device)
    check(lib().moc_nystrom_token_backward(ptr(qkv.detach()), n_pad, NYSTROM_HEADS, NYSTROM_DIM_HEAD, NYSTROM_LANDMARKS,
                                           ptr(k_l), ptr(Y), C.c_float(float(scale)), ptr(dout), ptr(dqkv), ptr(dk_l), ptr(dY),
                                           ptr(ws), nbytes, _stream()), "moc_nystrom_token_backward")
    return dqkv, dk_l, dY


def nystrom_conv_backward(qkv: torch.Tensor, conv_w: torch.Tensor, dout: torch.Tensor, dqkv: torch.Tensor) -> torch.Tensor:
    """Backward of nystrom_token_values' residual convolution (moc_nystrom_conv_backward): from qkv [n_pad, 1536], conv_w
    [8, taps] and dout [n_pad, 512] it WRITES dv into the v columns of the dqkv it is given (a contiguous [n_pad, 1536], e.g.
    nystrom_token_backward's: the q and k columns are left as they are) and returns dconv_w [8, taps]."""
    what = "nystrom_conv_backward"
    n_pad = _nystrom_qkv(qkv, what)
    for t in (conv_w, dout, dqkv):
        assert t.is_cuda and t.dtype == torch.float32, f"{what}: fp32 tensors on the GPU (no CPU fallback)"
    assert conv_w.dim() == 2 and conv_w.shape[0] == NYSTROM_HEADS, f"{what}: conv_w must be [8, taps]"
    taps = conv_w.shape[1]
    assert taps % 2 == 1 and taps <= NYSTROM_MAX_TAPS, f"{what}: taps={taps} must be odd and at most 33"
    assert dout.shape == (n_pad, NYSTROM_HEADS * NYSTROM_DIM_HEAD), f"{what}: dout must be [n_pad, 512]"
    assert dqkv.shape == qkv.shape and dqkv.is_contiguous() and not dqkv.requires_grad, \
        f"{what}: dqkv must be a contiguous [n_pad, 1536] that wants no gradient"
    conv_w, dout = conv_w.detach().contiguous(), dout.detach().contiguous()
    dconv_w = torch.empty_like(conv_w)
    nbytes = lib().moc_nystrom_conv_backward_workspace(n_pad, NYSTROM_HEADS, NYSTROM_DIM_HEAD, NYSTROM_LANDMARKS, taps)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=qkv.device)
    check(lib().moc_nystrom_conv_backward(ptr(qkv.detach()), n_pad, NYSTROM_HEADS, NYSTROM_DIM_HEAD, NYSTROM_LANDMARKS,
                                          ptr(conv_w), taps, ptr(dout), ptr(dqkv), ptr(dconv_w), ptr(ws), nbytes, _stream()),
          "moc_nystrom_conv_backward")
    return dconv_w


def nystrom_pinv(attn2: torch.Tensor, iters: int) -> torch.Tensor:
    """The landmark pseudo-inverse of the fused Nystrom forward (moc_nystrom_pinv): nystrom.moore_penrose_iter_pinv of
    attn2 [8, 256, 256] -- Z0 = attn2^T / (max row sum x max column sum of |attn2| over all heads), then `iters` times
    Z <- 1/4 Z (13 I - XZ (15 I - XZ (7 I - XZ))) -- as 2 + 4 iters launches of fp32 MFMA products.  No gradient."""
    what = "nystrom_pinv"
    assert attn2.is_cuda and attn2.dtype == torch.float32, f"{what}: fp32 tensors on the GPU (no CPU fallback)"
    assert attn2.shape == (NYSTROM_HEADS, NYSTROM_LANDMARKS, NYSTROM_LANDMARKS), f"{what}: attn2 must be [8, 256, 256]"
    iters = int(iters)
    assert 0 <= iters <= 64, f"{what}: iters={iters} must be in 0..64"
    attn2 = attn2.detach().contiguous()
    Z = torch.empty_like(attn2)
    nbytes = lib().moc_nystrom_pinv_workspace(NYSTROM_HEADS, NYSTROM_LANDMARKS)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=attn2.device)
    check(lib().moc_nystrom_pinv(ptr(attn2), NYSTROM_HEADS, NYSTROM_LANDMARKS, iters, ptr(Z), ptr(ws), nbytes, _stream()),
          "moc_nystrom_pinv")
    return Z


def _nystrom_mmm(t: torch.Tensor, name: str, what: str) -> torch.Tensor:
    assert t.is_cuda and t.dtype == torch.float32, f"{what}: fp32 tensors on the GPU (no CPU fallback)"
    assert t.shape == (NYSTROM_HEADS, NYSTROM_LANDMARKS, NYSTROM_LANDMARKS), f"{what}: {name} must be [8, 256, 256]"
    return t.detach().contiguous()


def nystrom_pinv_iterates(attn2: torch.Tensor, iters: int) -> torch.Tensor:
    """nystrom_pinv that keeps every iterate (moc_nystrom_pinv_iterates): Zs [iters + 1, 8, 256, 256] with Zs[t] = Z_t, and
    Zs[iters] bit for bit nystrom_pinv's result.  What nystrom_pinv_backward needs; no gradient of its own."""
    what = "nystrom_pinv_iterates"
    attn2 = _nystrom_mmm(attn2, "attn2", what)
    iters = int(iters)
    assert 0 <= iters <= 64, f"{what}: iters={iters} must be in 0..64"
    Zs = torch.empty((iters + 1,) + tuple(attn2.shape), dtype=torch.float32, device=attn2.device)
    nbytes = lib().moc_nystrom_pinv_workspace(NYSTROM_HEADS, NYSTROM_LANDMARKS)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=attn2.device)
    check(lib().moc_nystrom_pinv_iterates(ptr(attn2), NYSTROM_HEADS, NYSTROM_LANDMARKS, iters, ptr(Zs), ptr(ws), nbytes, _stream()),
          "moc_nystrom_pinv_iterates")
    return Zs


def nystrom_pinv_backward(attn2: torch.Tensor, Zs: torch.Tensor, dZ: torch.Tensor, iters: int) -> torch.Tensor:
    """The gradient through nystrom_pinv_iterates (moc_nystrom_pinv_backward): d attn2 [8, 256, 256] from attn2, its iterates
    Zs [iters + 1, 8, 256, 256] and dZ = d(Zs[iters]), the scaling by the two maximal sums included (ties share evenly, as
    torch's max() does).  3 + 4 iters product launches and four more; XZ, P2 and P3 are recomputed."""
    what = "nystrom_pinv_backward"
    attn2, dZ = _nystrom_mmm(attn2, "attn2", what), _nystrom_mmm(dZ, "dZ", what)
    iters = int(iters)
    assert 0 <= iters <= 64, f"{what}: iters={iters} must be in 0..64"
    assert Zs.is_cuda and Zs.dtype == torch.float32, f"{what}: fp32 tensors on the GPU (no CPU fallback)"
    assert Zs.shape == (iters + 1,) + tuple(attn2.shape), f"{what}: Zs must be [iters + 1, 8, 256, 256]"
    Zs = Zs.detach().contiguous()
    dA = torch.empty_like(attn2)
    nbytes = lib().moc_nystrom_pinv_backward_workspace(NYSTROM_HEADS, NYSTROM_LANDMARKS)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=attn2.device)
    check(lib().moc_nystrom_pinv_backward(ptr(attn2), NYSTROM_HEADS, NYSTROM_LANDMARKS, iters, ptr(Zs), ptr(dZ), ptr(dA), ptr(ws),
                                          nbytes, _stream()), "moc_nystrom_pinv_backward")
    return dA


NYSTROM_MAX_ROWS = 16                                                                  # rows per moc_nystrom_attention_rows call


def nystrom_attention_rows(qkv: torch.Tensor, q_l: torch.Tensor, lse: torch.Tensor, coef: torch.Tensor) -> torch.Tensor:
    """R rows of the layer's attention matrix attn1 pinv attn3 over all n_pad keys (moc_nystrom_attention_rows): out
    [8, R, n_pad] with out[h, r, j] = sum_m coef[h, r, m] exp(q_l[h, m] . k[j, h] - lse[h, m]), from qkv [n_pad, 1536], the
    scaled landmark queries q_l [8, 256, 64], nystrom_landmark_values_lse's lse [8, 256] for the same two, and coef
    [8, R, 256] = softmax_256(scale q[rows] k_l^T) pinv, 1 <= R <= NYSTROM_MAX_ROWS.  attn3 is not formed; no gradient."""
    what = "nystrom_attention_rows"
    n_pad = _nystrom_qkv(qkv, what)
    q_l = _nystrom_hmd(q_l, "q_l", what)
    assert lse.is_cuda and lse.dtype == torch.float32 and coef.is_cuda and coef.dtype == torch.float32, \
        f"{what}: fp32 tensors on the GPU (no CPU fallback)"
    assert lse.shape == (NYSTROM_HEADS, NYSTROM_LANDMARKS), f"{what}: lse must be [8, 256]"
    assert coef.dim() == 3 and coef.shape[0] == NYSTROM_HEADS and coef.shape[2] == NYSTROM_LANDMARKS \
        and 1 <= coef.shape[1] <= NYSTROM_MAX_ROWS, f"{what}: coef must be [8, R, 256] with R in 1..{NYSTROM_MAX_ROWS}"
    lse, coef = lse.detach().contiguous(), coef.detach().contiguous()
    R = coef.shape[1]
    out = torch.empty((NYSTROM_HEADS, R, n_pad), dtype=torch.float32, device=qkv.device)
    check(lib().moc_nystrom_attention_rows(ptr(qkv.detach()), n_pad, NYSTROM_HEADS, NYSTROM_DIM_HEAD, NYSTROM_LANDMARKS, ptr(q_l),
                                           ptr(lse), ptr(coef), R, ptr(out), _stream()), "moc_nystrom_attention_rows")
    return out


PPEG_DIM, PPEG_MAX_POSITIONS = 512, 1 << 22                                            # what moc_ppeg_* is built for


def _ppeg_tokens(t: torch.Tensor, H: int, W: int, name: str, what: str) -> torch.Tensor:
    assert t.is_cuda and t.dtype == torch.float32, f"{what}: fp32 tensors on the GPU (no CPU fallback)"
    assert H >= 1 and W >= 1 and H * W <= PPEG_MAX_POSITIONS, f"{what}: H={H} W={W} must be at least 1, H W at most 2^22"
    n = 1 + H * W
    assert t.shape in ((n, PPEG_DIM), (1, n, PPEG_DIM)), f"{what}: {name} must be [1 + H W, 512] (or [1, 1 + H W, 512])"
    return t.detach().contiguous()


def _ppeg_params(ws, bs, what: str):
    out = []
    for k, w in zip((7, 5, 3), ws):
        assert w.is_cuda and w.dtype == torch.float32, f"{what}: fp32 tensors on the GPU (no CPU fallback)"
        assert w.shape == (PPEG_DIM, 1, k, k), f"{what}: w{k} must be [512, 1, {k}, {k}]"
        out.append(w.detach().contiguous())
    for k, b in zip((7, 5, 3), bs):
        assert b.is_cuda and b.dtype == torch.float32, f"{what}: fp32 tensors on the GPU (no CPU fallback)"
        assert b.shape == (PPEG_DIM,), f"{what}: b{k} must be [512]"
        out.append(b.detach().contiguous())
    return out


def ppeg_forward(x: torch.Tensor, H: int, W: int, w7, b7, w5, b5, w3, b3) -> torch.Tensor:
    """TransMIL's PPEG in one launch (moc_ppeg_forward): from x [1 + H W, 512] (or [1, 1 + H W, 512]), row 0 the class token,
    and the three depth-wise convolutions' weights [512, 1, k, k] and biases [512], out of x's shape with
    out[0] = x[0], out[1 + p] = x[1 + p] + (b7 + b5 + b3) + the 7 x 7, 5 x 5 and 3 x 3 convolutions at position p.  No gradient."""
    what = "ppeg_forward"
    H, W = int(H), int(W)
    xc = _ppeg_tokens(x, H, W, "x", what)
    w7, w5, w3, b7, b5, b3 = _ppeg_params((w7, w5, w3), (b7, b5, b3), what)
    out = torch.empty_like(xc)
    check(lib().moc_ppeg_forward(ptr(xc), H, W, PPEG_DIM, ptr(w7), ptr(b7), ptr(w5), ptr(b5), ptr(w3), ptr(b3), ptr(out),
                                 _stream()), "moc_ppeg_forward")
    return out


def ppeg_backward(x: torch.Tensor, H: int, W: int, w7, w5, w3, dout: torch.Tensor):
    """Backward of ppeg_forward (moc_ppeg_backward): (dx, dw7, db7, dw5, db5, dw3, db3) from its x, its three weights and dout
    of x's shape.  dx has x's shape; the weight gradients are the three windows of one 7 x 7 table of sums and the three
    bias gradients are one sum, added in double above 64 products in a fixed order: two calls give the same bits."""
    what = "ppeg_backward"
    H, W = int(H), int(W)
    xc, dc = _ppeg_tokens(x, H, W, "x", what), _ppeg_tokens(dout, H, W, "dout", what)
    assert dc.shape == xc.shape, f"{what}: dout must have x's shape"
    w7, w5, w3 = _ppeg_params((w7, w5, w3), (), what)
    dx = torch.empty_like(xc)
    dw7, dw5, dw3 = torch.empty_like(w7), torch.empty_like(w5), torch.empty_like(w3)
    db7, db5, db3 = (torch.empty(PPEG_DIM, dtype=torch.float32, device=xc.device) for _ in range(3))
    nbytes = lib().moc_ppeg_backward_workspace(H, W, PPEG_DIM)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=xc.device)
    check(lib().moc_ppeg_backward(ptr(xc), H, W, PPEG_DIM, ptr(w7), ptr(w5), ptr(w3), ptr(dc), ptr(dx), ptr(dw7), ptr(db7),
                                  ptr(dw5), ptr(db5), ptr(dw3), ptr(db3), ptr(ws), nbytes, _stream()), "moc_ppeg_backward")
    return dx, dw7, db7, dw5, db5, dw3, db3
