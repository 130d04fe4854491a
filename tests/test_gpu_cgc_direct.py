"""The PLE level boundary (cdc_cgc_mid_fwd / _bwd, csrc/cgc.hip) and the narrow gate pooling (cdc_gate_pool_fwd / _bwd,
csrc/rowops.hip) straight through the C-ABI against tests/cgc_ref.py: a stage-wise float64 restatement with derived bounds, capped
by the suite's present figures.  The test builds cdc_cgc_mid_fwd_args, cdc_cgc_mid_bwd_args, cdc_pool_fwd_args and
cdc_pool_bwd_args itself: it writes the bf16 weights (w straight, wt transposed, the gates' wt zero-padded to 32 columns) from
bn_ref.bf16_bits and chooses every stride, flag and NULL pointer.  Buffers follow tests/test_gpu_tower_direct.py: NaN in input
padding, a sentinel that must survive in output padding and in two extra rows below row B of every output matrix, plain stores into
NaN, the accumulate target pre-filled with random values.  Padded leading dimensions keep the alignment the host entries demand
(multiples of 4 floats / 8 bf16 for the matrices; logits and their gradients take any stride: + 3).  The backward launches are given
ex2 and the probabilities of the float64 reference forward rounded to fp32 (cgc_ref.bwd_inputs), so a backward case does not hang on
its forward.  Every case has at most 67 rows.

Which case (cgc_ref.mid_cases / pool_cases) reaches which path of csrc/cgc.hip:
  * the PLE-3 layout (8, 4, 8, 3): ple3_b*; the second gate pass (ps == 1: more than 4 gates per level, both levels, both
    directions), the forward's extra-tile loop (12 x 4 + 5 = 53 jobs > 48), the backward's extra grad-input tiles (6 x 8 = 48 jobs >
    32) and its second expert chunk (n_exp = 12 > 8): tower5_b17, tower5_b35; both maxima (4, 8, 16, 8) — 64 + 8 = 72 forward jobs,
    153 600 bytes of LDS in the backward, exactly the limit: max_b16, max_b17; a single expert and gate with n_sel = 1
    (probabilities exactly 1, gate-logit gradients exactly 0): one_b1, one_b17;
  * a source with exactly MID_MAXSTEP = 6 K steps as three experts, as two experts + two gates, and a source with ONE K step (a
    single gate: the `sc` clamp of the grad-input tile): steps_b17, steps_b35, max_*;
  * n_sel = 16: max_* (level-k+1 gate 0); n_sel = 1 among longer lists: max_* (level-k gate 2), steps_*; non-prefix sel lists
    ({1, 3, 7}, {1, 2, 3, 7}), an expert every gate selects and one no gate selects (written as exactly 0): sparse_b17, max_*;
  * B = 1, 15, 16, 17, 35 (B not a multiple of 16, one and three workgroups): ple3_b1 .. ple3_b35;
  * drop_p 0 / 0.2 / 0.5: p0, most cases, p05 and steps_b35; seed_offset_dev NULL: nostep; a dropout stream per expert: every
    case (stream ids 67 + e); relu = 0: relu0; NULL biases: nobias; NULL pooled_h / out / out_h: null_pooled_h, null_out, null_out_h
    (each also bit-equal to ple3_b17 in what it does write); mask1 / mask2 off: mask1off, mask2off, relu0; scale1 != scale2 and
    neither the dropout scale: scales; d_logits_h present: ple3_b35, tower5_b17, max_b17;
  * padded leading dimensions: every case, as its padded launch.
Of csrc/rowops.hip (cdc_gate_pool_*): H = 4 (one lane per row), 64 and 128 (sub-wave), 256 (a full wave) take the 16-byte-lane
kernels; H = 12 (no power of two) and 320 (two passes) the scalar ones: h4 .. h320; an odd ld_exp forces the scalar kernels at
H = 64: h64_unaligned (its forward bit-equal to h64's); n_expert = 16, the 16-byte backward's limit (64 KB of LDS): e16; 17 and 32
(scalar backward): e17, e32; n_gates 1 and 16, n_sel 1 and 16: g1, g16, e16, e17; overlapping selections, a descending list and an
unselected expert: every case with the default lists; accumulate and mask_relu 0 / 1: acc1, acc1_h12, mask0, mask0_h320; B = 1, 5,
67: b1, most cases, b67*.

Bit equalities the code implies (assert_bits_equal): the padded against the tight layout and a second launch on the same inputs,
every case; rows 0..16 of the B = 17 launch against the same rows of the B = 35 launch (dropout is by global row); probs1 and
pooled_h of the fused forward against probs and out_h of cdc_gate_pool_fwd on the same inputs (the header's claim); the scalar
against the 16-byte pool forward; every bf16 shadow against the fp32 value beside it (cgc_ref.compare).  B = 0 returns 0 and writes
nothing."""
import ctypes as C

import numpy as np
import pytest
import torch

import cgc_ref as R
from helpers import OUT_SENTINEL, PadBuf, PadBufH, assert_bits_equal, nan_like

pytestmark = pytest.mark.gpu
MID, POOL = R.mid_cases(), R.pool_cases()
XR = 2                                          # sentinel rows below row B of every output matrix
_DATA, _RUNS = {}, {}


@pytest.fixture(scope="module")
def lib(cuda):
    from cdcmdr_amd import _lib as L
    return L.load()


def data(c):
    if c["name"] not in _DATA:
        D = R.make_data(c)
        D["I"] = R.pool_bwd_inputs(c, D) if c["op"] == "pool" else R.bwd_inputs(c, D)
        _DATA[c["name"]] = D
    return _DATA[c["name"]]


def ids(cs):
    return [c["name"] for c in cs]


class Rows:
    """an fp32 output matrix [B, cols] with XR sentinel rows below it, inside a PadBuf"""

    def __init__(self, dev, init, pad):
        init = np.asarray(init, dtype=np.float32)
        self.M = init.shape[0]
        self.b = PadBuf(dev, np.vstack([init, np.full((XR, init.shape[1]), OUT_SENTINEL, np.float32)]), out=True, pad=pad)
        self.ptr, self.ld = self.b.ptr, self.b.ld

    def read(self, what):
        h = self.b.read(what)
        assert (h[self.M:] == np.float32(OUT_SENTINEL)).all(), f"{what}: rows below B written"
        return h[:self.M]


class Launch:
    """fresh device buffers for one launch of a case in layout "t" (tight) or "p" (padded), and the argument block over them"""

    def __init__(self, lib, dev, c, fn, lay):
        from cdcmdr_amd import _lib as L
        self.L, self.lib, self.c, self.dev, self.fn = L, lib, c, dev, fn
        self.fp, self.hp, self.lp = (0, 0, 0) if lay == "t" else (4, 8, 3)
        self.keep, self.out = [], {}

    def k(self, b):
        self.keep.append(b)
        return b

    def inp(self, v, pad):
        return self.k(PadBuf(self.dev, np.asarray(v, dtype=np.float32), pad=pad))

    def vec(self, v):
        return self.k(PadBuf(self.dev, np.asarray(v, dtype=np.float32).reshape(1, -1))).ptr

    def inph(self, v):
        return self.k(PadBufH(self.dev, np.asarray(v, dtype=np.float32), pad=self.hp))

    def dense(self, v):
        """a contiguous fp32 input (the probabilities: [B, n_sel] without a stride)"""
        return self.k(torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(self.dev)).data_ptr()

    def rows(self, name, n, cols, pad, init=None):
        b = self.out[name] = Rows(self.dev, nan_like(n, cols) if init is None else init, pad)
        return b

    def rowsh(self, name, n, cols, pad):
        b = self.out[name] = PadBufH(self.dev, nan_like(n, cols), out=True, pad=pad, extra_rows=XR)
        return b

    def run(self):
        rc = getattr(self.lib, self.fn)(C.byref(self.a), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        self.L.check(rc, self.fn)
        torch.cuda.synchronize()
        return {name: b.read(f"{self.c['name']} {self.fn} {name}") for name, b in self.out.items()}


def mid_fwd(lib, dev, c, D, lay="t"):
    A = Launch(lib, dev, c, "cdc_cgc_mid_fwd", lay)
    a = A.a = R.mid_fwd_args(A.L.CgcMidFwdArgs(), c)
    ne1, ng1, ne2, ng2 = c["counts"]
    T, n = c["topo"], c["B"]
    ex1, ex2 = A.inp(D["ex1"], A.fp), A.rows("ex2", n, ne2 * R.H2, A.fp)
    a.ex1, a.ld_ex1, a.ex2, a.ld_ex2 = ex1.ptr, ex1.ld, ex2.ptr, ex2.ld
    if c["step"] is not None and c["p"] > 0:
        a.seed_offset_dev = A.k(torch.tensor([c["step"]], dtype=torch.int32, device=dev)).data_ptr()
    for g in range(ng1):
        G, ns = a.g1[g], len(T["sel1"][g])
        lg = A.inp(D["logits1"][g], A.lp)
        G.logits, G.ld_logits, G.probs = lg.ptr, lg.ld, A.rows(f"probs1_{g}", n, ns, 0).ptr
        if "pooled_h" not in c["null"]:
            ph = A.rowsh(f"pooled_h_{g}", n, R.H1, A.hp)
            G.pooled_h, G.ld_pooled_h = ph.ptr, ph.ld
    for e in range(ne2):
        w = A.inph(D["W"][e])
        a.e2[e].w, a.e2[e].ldw = w.ptr, w.ld
        if c["bias"]:
            a.e2[e].bias = A.vec(D["b"][e])
    for t in range(ng2):
        G, ns = a.g2[t], len(T["sel2"][t])
        w = A.inph(D["Wg"][t])
        G.w, G.ldw, G.probs = w.ptr, w.ld, A.rows(f"probs2_{t}", n, ns, 0).ptr
        if c["bias"]:
            G.bias = A.vec(D["bg"][t])
        if "out" not in c["null"]:
            o = A.rows(f"out_{t}", n, R.H2, A.fp)
            G.out, G.ld_out = o.ptr, o.ld
        if "out_h" not in c["null"]:
            oh = A.rowsh(f"outh_{t}", n, R.H2, A.hp)
            G.out_h, G.ld_out_h = oh.ptr, oh.ld
    return A


def mid_bwd(lib, dev, c, D, lay="t", I=None):
    A = Launch(lib, dev, c, "cdc_cgc_mid_bwd", lay)
    a = A.a = R.mid_bwd_args(A.L.CgcMidBwdArgs(), c)
    ne1, ng1, ne2, ng2 = c["counts"]
    T, n, I = c["topo"], c["B"], I or D["I"]
    ex1, ex2 = A.inp(D["ex1"], A.fp), A.inp(I["ex2"], A.fp)
    dz1, dz2 = A.rowsh("dz1_h", n, ne1 * R.H1, A.hp), A.rowsh("dz2_h", n, ne2 * R.H2, A.hp)
    a.ex1, a.ld_ex1, a.ex2, a.ld_ex2 = ex1.ptr, ex1.ld, ex2.ptr, ex2.ld
    a.dz1_h, a.ld_dz1_h, a.dz2_h, a.ld_dz2_h = dz1.ptr, dz1.ld, dz2.ptr, dz2.ld

    def dlogits(G, name, nameh, ns):
        d = A.rows(name, n, ns, A.lp)
        G.d_logits, G.ld_dlogits = d.ptr, d.ld
        if c["dlh"]:
            h = A.rowsh(nameh, n, ns, A.lp)
            G.d_logits_h, G.ld_dlogits_h = h.ptr, h.ld

    for g in range(ng1):
        a.g1[g].probs = A.dense(I["probs1"][g])
        dlogits(a.g1[g], f"dl1_{g}", f"dl1h_{g}", len(T["sel1"][g]))
    for e in range(ne2):
        wt = A.inph(np.asarray(D["W"][e]).T)
        a.e2[e].wt, a.e2[e].ldwt = wt.ptr, wt.ld
    for t in range(ng2):
        G, ns = a.g2[t], len(T["sel2"][t])
        do = A.inp(D["dout"][t], A.fp)
        wt = np.zeros((R.H1, 32), np.float32)
        wt[:, :ns] = np.asarray(D["Wg"][t]).T
        wtb = A.inph(wt)
        G.d_out, G.ld_dout, G.probs, G.wt, G.ldwt = do.ptr, do.ld, A.dense(I["probs2"][t]), wtb.ptr, wtb.ld
        dlogits(G, f"dl2_{t}", f"dl2h_{t}", ns)
    return A


def pool_fwd(lib, dev, c, D, lay="t"):
    A = Launch(lib, dev, c, "cdc_gate_pool_fwd", lay)
    a = A.a = R.pool_args(A.L.PoolFwdArgs(), c)
    n, H = c["B"], c["H"]
    ex = A.inp(D["ex"], 3 if c["unaligned"] else A.fp)
    a.experts, a.ld_exp = ex.ptr, ex.ld
    for g, sel in enumerate(c["sels"]):
        G = a.gate[g]
        lg, o, oh = A.inp(D["logits"][g], A.lp), A.rows(f"out_{g}", n, H, A.fp), A.rowsh(f"outh_{g}", n, H, A.hp)
        G.logits, G.ld_logits, G.out, G.ld_out, G.out_h, G.ld_out_h = lg.ptr, lg.ld, o.ptr, o.ld, oh.ptr, oh.ld
        G.probs = A.rows(f"probs_{g}", n, len(sel), 0).ptr
    return A


def pool_bwd(lib, dev, c, D, lay="t"):
    A = Launch(lib, dev, c, "cdc_gate_pool_bwd", lay)
    a = A.a = R.pool_args(A.L.PoolBwdArgs(), c)
    n, H, E = c["B"], c["H"], c["n_expert"]
    ex = A.inp(D["ex"], 3 if c["unaligned"] else A.fp)
    dex, dexh = A.rows("dex", n, E * H, A.fp, D["dex0"] if c["acc"] else None), A.rowsh("dexh", n, E * H, A.hp)
    a.experts, a.ld_exp, a.d_experts, a.ld_dexp, a.d_experts_h, a.ld_dexp_h = ex.ptr, ex.ld, dex.ptr, dex.ld, dexh.ptr, dexh.ld
    for g, sel in enumerate(c["sels"]):
        G = a.gate[g]
        do, d, h = A.inp(D["dout"][g], A.fp), A.rows(f"dl_{g}", n, len(sel), A.lp), A.rowsh(f"dlh_{g}", n, len(sel), A.lp)
        G.d_out, G.ld_dout, G.probs = do.ptr, do.ld, A.dense(D["I"]["probs"][g])
        G.d_logits, G.ld_dlogits, G.d_logits_h, G.ld_dlogits_h = d.ptr, d.ld, h.ptr, h.ld
    return A


BUILD = {"mid": (mid_fwd, mid_bwd), "pool": (pool_fwd, pool_bwd)}


def launches(lib, dev, c, lay="t", cache=True):
    """(forward outputs, backward outputs) of a case; the tight launch of a case is run once and shared, never changed"""
    key = (c["name"], lay)
    if not cache or key not in _RUNS:
        D = data(c)
        res = tuple(build(lib, dev, c, D, lay).run() for build in BUILD[c["op"]])
        if not cache:
            return res
        _RUNS[key] = res
    return _RUNS[key]


def same_bits(a, b, what, rows=None):
    assert a.keys() == b.keys(), (what, a.keys() ^ b.keys())
    for k in a:
        assert_bits_equal(a[k][:rows], b[k][:rows], f"{what} {k}")


# ------------------------------------------------------------------------------------------------------------------------
# both directions against float64, every case
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", MID, ids=ids(MID))
def test_level_boundary_against_float64(cuda, lib, c):
    D = data(c)
    assert lib.cdc_cgc_mid_fits(*c["counts"]) == 1
    f, b = launches(lib, cuda, c)
    fill = None
    if c["null"]:                                                    # what the case does write: the bits of the launch with every output
        fill = launches(lib, cuda, R.by_name("ple3_b17"))[0]
        same_bits(f, {k: fill[k] for k in f}, f"{c['name']} against ple3_b17")
    F = R.ref_mid_fwd(c, D, R.saved_fwd(c, f, fill))
    R.compare(f, F, f"{c['name']} fwd")
    Bk = R.ref_mid_bwd(c, D, D["I"], R.saved_bwd(c, b))
    R.compare(b, Bk, f"{c['name']} bwd")
    assert set(f) == set(R.rounded(c, F)) and set(b) == set(R.rounded(c, Bk))
    if c["kind"] == "one":                                           # n_sel = 1: probabilities exactly 1, gate-logit gradients exactly 0
        assert (f["probs1_0"] == 1).all() and (f["probs2_0"] == 1).all() and not b["dl1_0"].any() and not b["dl2_0"].any()
    if c["kind"] == "sparse":                                        # experts 0, 5, 6: selected by no gate
        for e in (0, 5, 6):
            assert not b["dz2_h"][:, e * R.H2:(e + 1) * R.H2].any() and not b["dz1_h"][:, e * R.H1:(e + 1) * R.H1].any()
    if c["p"] > 0:
        assert ((f["ex2"] == 0) & (F["ex2"][1] == 0)).mean() > c["p"] / 2


@pytest.mark.parametrize("c", POOL, ids=ids(POOL))
def test_gate_pool_against_float64(cuda, lib, c):
    D = data(c)
    f, b = launches(lib, cuda, c)
    F = R.ref_pool_fwd(c, D, R.saved_fwd(c, f))
    R.compare(f, F, f"{c['name']} fwd")
    Bk = R.ref_pool_bwd(c, D, D["I"])
    R.compare(b, Bk, f"{c['name']} bwd")
    assert set(f) == set(R.rounded(c, F)) and set(b) == set(R.rounded(c, Bk))
    if c["sels"][:3] == [[0, 1], [1, 3], [3, 1, 0]] and not c["acc"]:                          # expert 2: selected by no gate
        assert not b["dex"][:, 2 * c["H"]:3 * c["H"]].any()


# ------------------------------------------------------------------------------------------------------------------------
# bit equalities
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", MID + POOL, ids=ids(MID + POOL))
def test_padded_layout_and_second_launch_give_the_same_bits(cuda, lib, c):
    f, b = launches(lib, cuda, c)
    for lay, what in (("p", "padded"), ("t", "second launch")):
        f2, b2 = launches(lib, cuda, c, lay, cache=False)
        same_bits(f2, f, f"{c['name']} {what}, forward")
        same_bits(b2, b, f"{c['name']} {what}, backward")


def test_a_row_does_not_depend_on_the_batch(cuda, lib):
    small, big = R.by_name("ple3_b17"), R.by_name("ple3_b35")
    D, Db = data(small), data(big)
    fb, bb = launches(lib, cuda, big)
    f = mid_fwd(lib, cuda, dict(small, dlh=True), D).run()
    I = dict(ex2=Db["I"]["ex2"][:17], probs1=[v[:17] for v in Db["I"]["probs1"]], probs2=[v[:17] for v in Db["I"]["probs2"]])
    b = mid_bwd(lib, cuda, dict(small, dlh=True), D, I=I).run()
    same_bits(f, {k: v[:17] for k, v in fb.items()}, "rows 0..16 of 35, forward")
    same_bits(b, {k: v[:17] for k, v in bb.items()}, "rows 0..16 of 35, backward")
    assert (fb["ex2"][17:] == 0).any() and np.isfinite(fb["ex2"]).all()


@pytest.mark.parametrize("name", ["ple3_b17", "tower5_b35", "max_b17"])
def test_fused_forward_gives_the_pool_forwards_bits(cuda, lib, name):
    c = R.by_name(name)
    D = data(c)
    f, _ = launches(lib, cuda, c)
    T = c["topo"]
    cp = R.pool(f"{name}_level_k", H=R.H1, B=c["B"], n_expert=c["counts"][0], sels=T["sel1"])
    g = pool_fwd(lib, cuda, cp, dict(ex=D["ex1"], logits=D["logits1"])).run()
    for i in range(c["counts"][1]):
        assert_bits_equal(f[f"probs1_{i}"], g[f"probs_{i}"], f"{name} probs of gate {i}")
        assert_bits_equal(f[f"pooled_h_{i}"], g[f"outh_{i}"], f"{name} pooled_h of gate {i}")


def test_scalar_pool_forward_gives_the_16_byte_forms_bits(cuda, lib):
    f, _ = launches(lib, cuda, R.by_name("h64"))
    fs, _ = launches(lib, cuda, R.by_name("h64_unaligned"))
    same_bits(fs, f, "scalar against 16-byte lanes")


@pytest.mark.parametrize("op", ["mid", "pool"])
def test_an_empty_batch_returns_zero_and_writes_nothing(cuda, lib, op):
    c = R.by_name("ple3_b1" if op == "mid" else "b1")
    for build in BUILD[op]:
        A = build(lib, cuda, c, data(c))
        A.a.B = 0
        for k, v in A.run().items():                                 # (read() has checked the padding and the rows below B)
            assert v.shape[0] == 1 and np.isnan(v).all(), f"{A.fn} B = 0: {k} written"
