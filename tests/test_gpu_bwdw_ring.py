"""The operand ring of the shadow grad-weight kernels (csrc/gemm2.hip: g2_tn_body) at the shapes where a ring can go wrong,
through cdc_glinear_bwd_w and cdc_glinear_bwd_w_pair against tests/glinear_ref.py (float64, its bounds).  Since the fragment
reads are inline assembly, nothing but the K loop's own counted wait and barrier orders them behind the direct-to-LDS loads: a
mistake there is an LDS race inside a workgroup and shows as wrong or changing numbers.

The stages in the tree are 64 batch rows; a row slice of r rows is n = ceil(r / 64) of them.  The ring depths are D = 2 (wide
class, 128 x 128 tiles) and D = 3 (narrow class, 64 x 64 tiles).  Rows 64 ... 448 in steps of 64 with split_k = 1 are
n = 1 ... 7: fewer than D - 1 where that exists (the prologue must not issue past the end), D - 1, D, D + 1 and 2 D + 1 of
both depths (and of the 32-row rings of 4, 5 and 6 stages that were measured against them, profiles/round8/README.md: there
n doubles).  Ragged rows (1, 65, 100, 321): the rest of the last 64-row slab and everything past M is the shadows' zero
padding.  Slices: M = 65 in 2 and 3 slices (64, 1 and 0 rows: the empty slice writes an all-zero slab), M = 448 in 3
(192, 192, 64).

Every launch holds several groups (find_group and g_off), with and without db; with split_k = 1 one group accumulates.
Every case asserts: (1) dW, db and every slab within glinear_ref's bounds of float64; (2) the single launches and the pair
launch bit-equal; (3) the slabs of a defer_reduce launch summed on the host in slice order bit-equal to the reduced result;
(4) two runs into fresh buffers bit-equal (an LDS race inside a workgroup shows as a difference); (5) a guard region of a NaN
pattern on both sides of every output and of the workspace comes back unchanged."""
import ctypes as C

import numpy as np
import pytest
import torch

import glinear_ref as R
from bn_ref import bf16_round
from helpers import assert_bits_equal, assert_bounded

pytestmark = pytest.mark.gpu

GUARD = 64                                  # floats on each side
GUARD_BITS = 0x7FC0BEEF                     # a quiet NaN with a payload no kernel produces
WIDE = [(128, 128, 1, 0), (130, 72, 0, 0), (256, 416, 1, 0)]                      # (N, K, db, accumulate)
NARROW = [(4, 416, 1, 0), (32, 64, 0, 0), (64, 64, 1, 0), (64, 128, 1, 0)]
CASES = [(m, 1) for m in (64, 128, 192, 256, 320, 384, 448, 1, 65, 100, 321)] + [(65, 2), (65, 3), (448, 3)]
_REF = {}


@pytest.fixture(scope="module")
def lib(cuda):
    from cdcmdr_amd import _lib as L
    return L.load()


def call(lib, name, *args):
    from cdcmdr_amd import _lib as L
    L.check(getattr(lib, name)(*args, C.c_void_p(torch.cuda.current_stream().cuda_stream)), name)


def case(cls, M, split, defer):
    shapes = WIDE if cls == "wide" else NARROW
    groups = [(M, N, K, db, 1 if (split == 1 and i == 1) else acc, 0) for i, (N, K, db, acc) in enumerate(shapes)]
    return R.bwdw_case(f"ring_{cls}_{M}", groups, split=split, defer=defer)


def ref(c):
    """data and float64 reference of a case (the data does not depend on split / defer: make_data is seeded by the name)"""
    key = (c["name"], c["split"], c["defer"])
    if key not in _REF:
        if ("data", c["name"]) not in _REF:
            _REF["data", c["name"]] = R.make_data(c)
        D = _REF["data", c["name"]]
        _REF[key] = (D, R.ref_bwdw(c, D, R.BF16, 64, db_rounded=True))
    return _REF[key]


class Guarded:
    """`values` (fp32, any shape) between two guard regions"""

    def __init__(self, dev, values):
        v = np.ascontiguousarray(values, dtype=np.float32)
        self.shape, self.n = v.shape, v.size
        h = np.full(self.n + 2 * GUARD, 0, dtype=np.uint32)
        h[:] = GUARD_BITS
        h[GUARD:GUARD + self.n] = v.ravel().view(np.uint32)
        self.t = torch.from_numpy(h.view(np.float32)).to(dev)
        self.ptr = self.t.data_ptr() + 4 * GUARD

    def read(self, what):
        h = self.t.cpu().numpy().view(np.uint32)
        assert (h[:GUARD] == GUARD_BITS).all() and (h[GUARD + self.n:] == GUARD_BITS).all(), f"{what}: written outside the buffer"
        return h[GUARD:GUARD + self.n].view(np.float32).reshape(self.shape).copy()


def shadow(dev, values, rows):
    """bf16 copy as plan.py allocates shadows: rows to a multiple of 64 and columns to one plus 64; rows past `rows` zero, the
    column padding of the live rows NaN (nothing may leak from it)"""
    v = np.asarray(values, dtype=np.float32)[:rows]
    r64 = lambda n: (n + 63) // 64 * 64
    s = torch.zeros((r64(max(rows, 1)), r64(v.shape[1]) + 64), dtype=torch.bfloat16, device=dev)
    s[:rows, v.shape[1]:] = float("nan")
    s[:rows, :v.shape[1]] = torch.from_numpy(bf16_round(v)).to(dev).to(torch.bfloat16)
    return s


class Launch:
    """argument block and guarded buffers of one grad-weight launch over bf16 shadows"""

    def __init__(self, dev, c, D):
        from cdcmdr_amd import _lib as L
        self.c, self.a, self.keep, self.DW, self.DB = c, L.LinBwdwArgs(), [], [], []
        a = self.a
        a.n_groups, a.split_k, a.defer_reduce = len(c["groups"]), c["split"], c["defer"]
        self.stride = R.slab_layout(c)[1]
        self.ws = None
        if c["split"] > 1:
            self.ws = Guarded(dev, np.full((c["split"], self.stride), np.nan, np.float32))
            a.workspace = self.ws.ptr
        for g, (M, N, K, has_db, acc, _e) in enumerate(c["groups"]):
            start = acc or c["defer"]          # an accumulate target and what a deferred launch must leave alone start from values
            self.DW.append(Guarded(dev, D["dw0"][g] if start else np.full((N, K), np.nan, np.float32)))
            self.DB.append(Guarded(dev, D["db0"][g] if start else np.full(N, np.nan, np.float32)) if has_db else None)
            dz = torch.from_numpy(np.ascontiguousarray(D["dz"][g][:max(M, 1)])).to(dev)
            x = torch.from_numpy(np.ascontiguousarray(D["x"][g][:max(M, 1)])).to(dev)
            dzh, xh = shadow(dev, D["dz"][g], M), shadow(dev, D["x"][g], M)
            G = a.g[g]
            G.dz, G.lddz, G.x, G.ldx, G.dw, G.lddw = dz.data_ptr(), N, x.data_ptr(), K, self.DW[g].ptr, K
            G.M, G.N, G.K, G.accumulate = M, N, K, acc
            if has_db:
                G.db = self.DB[g].ptr
            G.dzh, G.lddzh, G.xh, G.ldxh = dzh.data_ptr(), dzh.stride(0), xh.data_ptr(), xh.stride(0)
            self.keep += [dz, x, dzh, xh]

    def results(self):
        torch.cuda.synchronize()
        out = {}
        for g, (M, N, K, has_db, *_r) in enumerate(self.c["groups"]):
            out[f"dw{g}"] = self.DW[g].read(f"{self.c['name']} dw{g}")
            if has_db:
                out[f"db{g}"] = self.DB[g].read(f"{self.c['name']} db{g}")
        if self.ws is not None:
            out["slabs"] = self.ws.read(f"{self.c['name']} workspace")
        return out


def single(lib, dev, c, D):
    w = Launch(dev, c, D)
    call(lib, "cdc_glinear_bwd_w", C.byref(w.a), R.BF16)
    return w.results()


def same_bits(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        x, y = np.nan_to_num(a[k], nan=0.0), np.nan_to_num(b[k], nan=0.0)      # (the db piece of a slab of a group without db)
        assert np.array_equal(np.isnan(a[k]), np.isnan(b[k])), f"{what} {k}: NaN pattern differs"
        assert_bits_equal(x, y, f"{what} {k}")


def check_slabs(c, got, want, what):
    sw, sb = R.slab_sums(c, want, want)
    ok = np.isfinite(sw)
    assert_bounded(got[ok], sw[ok], sb[ok], f"{what} slabs")
    for s, (_r0, rn) in enumerate(R.slices(c["groups"][0][0], c["split"], 64)):
        if rn == 0:                                               # the empty slice: all zero, not merely small
            assert not got[s][ok[s]].any(), f"{what}: slab {s} of an empty slice is not zero"


def host_reduce(slabs):
    s = np.zeros(slabs.shape[1:], np.float32)
    for k in range(slabs.shape[0]):
        s = s + slabs[k]
    return s


@pytest.mark.parametrize("M,split", CASES, ids=[f"M{m}-S{s}" for m, s in CASES])
def test_ring(cuda, lib, M, split):
    reduced, deferred = {}, {}
    for cls in ("wide", "narrow"):
        c = case(cls, M, split, 0)
        D, want = ref(c)
        got = single(lib, cuda, c, D)
        for k, (w, b) in want.items():                            # (1) float64
            if not k.startswith("slab"):
                assert_bounded(got[k], w, b, f"{c['name']} {k}")
        if split > 1:
            check_slabs(c, got["slabs"], want, c["name"])
        same_bits(got, single(lib, cuda, c, D), f"{c['name']} run 2")          # (4)
        reduced[cls] = got
        if split > 1:
            cd = case(cls, M, split, 1)
            Dd, wantd = ref(cd)
            d = single(lib, cuda, cd, Dd)
            off, _ = R.slab_layout(cd)
            for g, (_M, N, K, has_db, *_r) in enumerate(cd["groups"]):
                assert_bits_equal(d[f"dw{g}"], Dd["dw0"][g], f"{cd['name']}: dw{g} written by a deferred launch")
                assert_bits_equal(host_reduce(d["slabs"][:, off[g][0]:off[g][0] + N * K]).reshape(N, K), got[f"dw{g}"],
                                  f"{cd['name']} dw{g}: slabs summed in slice order")     # (3)
                if has_db:
                    assert_bits_equal(d[f"db{g}"], Dd["db0"][g], f"{cd['name']}: db{g} written by a deferred launch")
                    assert_bits_equal(host_reduce(d["slabs"][:, off[g][1]:off[g][1] + N]), got[f"db{g}"], f"{cd['name']} db{g}: slabs summed")
            check_slabs(cd, d["slabs"], wantd, cd["name"])
            same_bits({"slabs": d["slabs"]}, {"slabs": got["slabs"]}, f"{cd['name']} deferred against reduced")
            deferred[cls] = d
    # (2) the pair launch: both classes in one launch (it never reduces: its blocks are deferred when they are split)
    cs = [case(cls, M, split, 1 if split > 1 else 0) for cls in ("wide", "narrow")]
    pair = [Launch(cuda, c, ref(c)[0]) for c in cs]
    t = torch.frombuffer(bytearray(bytes(pair[0].a) + bytes(pair[1].a)), dtype=torch.uint8).to(cuda)
    call(lib, "cdc_glinear_bwd_w_pair", C.byref(pair[0].a), C.byref(pair[1].a), C.c_void_p(t.data_ptr()))
    for cls, w in zip(("wide", "narrow"), pair):
        same_bits(w.results(), deferred[cls] if split > 1 else reduced[cls], f"pair {cls} M={M} S={split}")
