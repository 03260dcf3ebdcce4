"""Host-side checks of the selected-row mailbox (moc_batch_t.n_sel_mail / n_sel_ticket): the two fields sit at the end of
the struct where the ctypes mirror puts them, and the step counters answer without a GPU."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mailbox_fields_end_the_struct_where_the_binding_puts_them(tmp_path):
    from moc_amd import _lib
    prog = tmp_path / "mail.c"
    prog.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "moc_hip.h"\n'
        "int main(void){\n"
        ' printf("%zu %zu %zu %zu %zu\\n", sizeof(moc_batch_t), offsetof(moc_batch_t, n_sel_host), offsetof(moc_batch_t, n_sel_mail),\n'
        "        offsetof(moc_batch_t, n_sel_ticket), sizeof(((moc_batch_t*)0)->n_sel_mail[0]));\n"
        " return 0;}\n")
    exe = tmp_path / "mail"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).decode().split()]
    B = _lib.MocBatch
    assert got == [ctypes.sizeof(B), B.n_sel_host.offset, B.n_sel_mail.offset, B.n_sel_ticket.offset, 8]
    assert [n for n, _ in B._fields_][-3:] == ["n_sel_host", "n_sel_mail", "n_sel_ticket"]
    assert B().n_sel_mail is None and B().n_sel_ticket == 0          # a zero-filled struct: no mailbox, no ticket


def test_step_counters_read_and_reset_without_a_gpu():
    from moc_amd import _lib
    h = _lib.lib()
    known, steps = ctypes.c_int64(-1), ctypes.c_int64(-1)
    assert h.moc_n_sel_stats(ctypes.byref(known), ctypes.byref(steps), 1) == 0
    assert known.value >= 0 and steps.value >= known.value
    assert h.moc_n_sel_stats(ctypes.byref(known), ctypes.byref(steps), 0) == 0
    assert (known.value, steps.value) == (0, 0)
    assert h.moc_n_sel_stats(None, None, 0) == 0                     # either pointer may be NULL


def test_ticket_counter_starts_at_one_and_skips_zero():
    """SlideBatch._n_sel_stale, the arithmetic alone (no device): 1, 2, ... and 0xFFFFFFFF -> 1."""
    from moc_amd import engine as E

    class Stub:
        _n_sel_stale = E.SlideBatch._n_sel_stale

        def __init__(self, ticket):
            self.c = E.MocBatch()
            self._n_sel_mail = E.torch.zeros(2, dtype=E.torch.int64)
            self._n_sel_ticket = ticket

    s = Stub(0)
    s._n_sel_stale()
    assert s._n_sel_ticket == s.c.n_sel_ticket == 1 and s.c.n_sel_mail == s._n_sel_mail.data_ptr() and s.c.n_sel_host is None
    s = Stub(0xFFFFFFFE)
    s._n_sel_stale()
    assert s.c.n_sel_ticket == 0xFFFFFFFF
    s._n_sel_stale()
    assert s._n_sel_ticket == s.c.n_sel_ticket == 1
