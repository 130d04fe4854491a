"""CPU-only checks of the wide gate-pooling entry points (include/cdcmdr.h cdc_gate_pool_wide_*): struct layouts against the
C compiler, limits, the host-side table packing, and the bad-argument paths (they return before anything is launched)."""
import ctypes as C
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cdcmdr.h")
STRUCTS = {"cdc_pool_wide_fwd_args": "PoolWideFwdArgs", "cdc_pool_wide_bwd_args": "PoolWideBwdArgs"}


def _lib():
    from cdcmdr_amd import _lib as L
    return L, L.load()


def test_wide_pool_layouts_and_limits_match_the_header():
    import re
    L, _ = _lib()
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void) {"]
    for cname, pyname in STRUCTS.items():
        last = getattr(L, pyname)._fields_[-1][0]
        lines.append(f'  printf("{cname} %zu %zu %zu\\n", sizeof({cname}), offsetof({cname}, {last}), sizeof((({cname}*)0)->{last}[0]));')
    lines += ["  return 0;", "}"]
    with tempfile.TemporaryDirectory() as td:
        src, exe = os.path.join(td, "abi.c"), os.path.join(td, "abi")
        open(src, "w").write("\n".join(lines))
        subprocess.run(["gcc", "-std=c11", "-o", exe, src], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    for line in out.strip().splitlines():
        cname, size, off, gate = line.split()
        cls = getattr(L, STRUCTS[cname])
        last = cls._fields_[-1][0]
        assert C.sizeof(cls) == int(size) and getattr(cls, last).offset == int(off), cname
        assert C.sizeof(dict(cls._fields_)[last]._type_) == int(gate), cname
        assert C.sizeof(cls) <= 4096, f"{cname} travels as a kernel argument and must stay under 4 KB"
    src = open(HEADER).read()
    for macro, val in [("CDC_WIDE_MAX_SEL", L.WIDE_MAX_SEL), ("CDC_WIDE_MAX_GATES", L.WIDE_MAX_GATES),
                       ("CDC_WIDE_MAX_EXPERT", L.WIDE_MAX_EXPERT)]:
        m = re.search(rf"#define\s+{macro}\s+(\d+)", src)
        assert m and int(m.group(1)) == val, macro
    assert L.WIDE_MAX_SEL >= 256 and L.WIDE_MAX_SEL > L.MAX_SEL


def _pack(lib, n_expert, sels, cap=None):
    n_sel = (C.c_int32 * len(sels))(*[len(s) for s in sels])
    flat = [int(e) for s in sels for e in s]
    sel = (C.c_int32 * max(len(flat), 1))(*flat)
    n = lib.cdc_gate_pool_wide_table(len(sels), n_expert, n_sel, sel, None, 0)
    if n <= 0:
        return n, None
    tab = (C.c_int32 * n)()
    rc = lib.cdc_gate_pool_wide_table(len(sels), n_expert, n_sel, sel, tab, n if cap is None else cap)
    return rc, list(tab)


def test_wide_table_packing():
    """selection offsets, the selections, and per expert its (gate, slot) entries in (gate, slot) order: the order the
    backward sums d_experts in"""
    _, lib = _lib()
    sels = [[4, 0, 2], [2, 3, 4, 4 - 4], [1]]
    n, t = _pack(lib, 6, sels)
    ng, ne, total = 3, 6, 8
    assert n == ng + ne + 2 + 2 * total == len(t)
    assert t[:ng + 1] == [0, 3, 7, 8]
    inv_off = t[ng + 1:ng + ne + 2]
    sel = t[ng + ne + 2:ng + ne + 2 + total]
    inv = t[ng + ne + 2 + total:]
    assert sel == [4, 0, 2, 2, 3, 4, 0, 1]
    assert inv_off == [0, 2, 3, 5, 6, 8, 8]                   # expert 5 is selected by no gate
    dec = [(v >> 16, v & 0xFFFF) for v in inv]
    assert dec == [(0, 1), (1, 3), (2, 0), (0, 2), (1, 0), (1, 1), (0, 0), (1, 2)]


def test_wide_table_fifty_domains():
    """PLE with 50 towers, level 1: 50 specific gates of 4 experts and the shared gate over all 102"""
    _, lib = _lib()
    n, ns, nsh = 50, 2, 2
    shared = [n * ns + k for k in range(nsh)]
    sels = [[i * ns + k for k in range(ns)] + shared for i in range(n)] + [list(range(n * ns + nsh))]
    for c0 in range(0, len(sels), 32):
        chunk = sels[c0:c0 + 32]
        rc, t = _pack(lib, n * ns + nsh, chunk)
        assert rc == len(t) > 0
        ne = n * ns + nsh
        inv_off = t[len(chunk) + 1:len(chunk) + ne + 2]
        assert inv_off[-1] == sum(len(s) for s in chunk)


@pytest.mark.parametrize("case", ["n_sel0", "n_sel_big", "sel_neg", "sel_high", "no_gates", "too_many_gates", "short_table",
                                  "experts_big"])
def test_wide_table_bad_arguments(case):
    L, lib = _lib()
    sels, n_expert, cap = [[0, 1, 2]], 4, None
    if case == "n_sel0":
        sels = [[0, 1], []]
    elif case == "n_sel_big":
        sels, n_expert = [list(range(L.WIDE_MAX_SEL + 1))], L.WIDE_MAX_SEL + 1
    elif case == "sel_neg":
        sels = [[0, -1]]
    elif case == "sel_high":
        sels = [[0, 4]]
    elif case == "no_gates":
        sels = []
    elif case == "too_many_gates":
        sels = [[0]] * (L.WIDE_MAX_GATES + 1)
    elif case == "short_table":
        cap = 5
    elif case == "experts_big":
        n_expert = L.WIDE_MAX_EXPERT + 1
    rc, _ = _pack(lib, n_expert, sels, cap)
    assert rc == -1, (case, rc)
    assert lib.cdc_last_error()


@pytest.mark.parametrize("which", ["fwd", "bwd"])
@pytest.mark.parametrize("case", ["n_sel0", "n_sel_big", "no_table", "n_gates0", "n_gates_big", "n_expert_big"])
def test_wide_pool_launch_bad_arguments(which, case):
    """argument checks of cdc_gate_pool_wide_fwd / _bwd: CDC_E_BADARG before any launch (the pointers are never dereferenced)"""
    L, lib = _lib()
    a = L.PoolWideFwdArgs() if which == "fwd" else L.PoolWideBwdArgs()
    dummy = 256
    a.n_gates, a.n_expert, a.H, a.B, a.experts, a.ld_exp, a.table = 1, 8, 16, 4, dummy, 128, dummy
    G = a.gate[0]
    if which == "fwd":
        G.logits, G.out, G.probs = dummy, dummy, dummy
    else:
        a.d_experts = dummy
        G.d_out, G.probs, G.d_logits = dummy, dummy, dummy
    G.n_sel = 8
    if case == "n_sel0":
        G.n_sel = 0
    elif case == "n_sel_big":
        G.n_sel = L.WIDE_MAX_SEL + 1
    elif case == "no_table":
        a.table = None
    elif case == "n_gates0":
        a.n_gates = 0
    elif case == "n_gates_big":
        a.n_gates = L.WIDE_MAX_GATES + 1
    elif case == "n_expert_big":
        a.n_expert = L.WIDE_MAX_EXPERT + 1
    fn = lib.cdc_gate_pool_wide_fwd if which == "fwd" else lib.cdc_gate_pool_wide_bwd
    assert fn(C.byref(a), None) == -1
