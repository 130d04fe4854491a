"""The fused tower launches of csrc/tower.hip (cdc_tower_fwd, cdc_tower_bwd, cdc_tower_step, cdc_tower_dp) straight through the
C-ABI against tests/tower_ref.py: a stage-wise float64 restatement with derived bounds, capped by the suite's present figures.
The test builds cdc_tower_args itself: it writes the bf16 operands (xh, wh with rows in whole 64-element slabs, wt the transposed
copy zero-padded to 64 columns) from bn_ref.bf16_bits and chooses every stride, flag and NULL pointer.  Buffers follow
tests/test_gpu_head.py: NaN in input padding, a sentinel that must survive in output padding and in two extra rows below row M of
every output matrix (z, a1h, a2, out, dzh, dx, wide_dx), plain stores into NaN, accumulate targets pre-filled with random values.
Padded leading dimensions are multiples of 4 floats / 8 bf16, as tower_check asks.  The workspace has
cdc_tower_workspace_bytes() bytes, 128-byte aligned, zeroed once per case; `err` must read 0 after EVERY launch (Launch.run): a set
CDC_TOWER_ERR_TIMEOUT fails the test, nothing is retried.

Which case (tower_ref.cases) reaches which path, and how the test knows:
  * chunk / block boundaries, a one-row last block, odd chunk counts: rows{2,63,64,65,127,128,129,193,257}_{dout,bce} (the row
    count IS the geometry: 64-row chunks, 128-row blocks); H0 = 128 (the two-slab instantiation): h128_65, h128_257;
  * n_tower 1, 2, 4: nt1, nt2, nt4; relu 0: relu0; sigmoid 0: nosig (d_out form); drop_p 0 / 0.2 / 0.5: p0, every rows* case, p05;
    seed_offset_dev NULL: nostep; bo / running_mean / num_batches_tracked NULL: nobo, norun, nonbt; each nullable output NULL:
    null_*; accumulate_dx mixed per tower: accdx, h128_257; accumulate_wide_dx: accwide, accwide_bce, wide512;
  * no wide term: wide0; wide_K 4, 28 (every other case), 256 (the whole first quad of a lane), 260 (one lane of the second
    quad), 512 (both quads full): wide4, wide256, wide260, wide512; wide_bias NULL: nowb; ld_wide > wide_K: the padded layout of each;
  * tw_gather_sums<64> second batch of 16 (65 chunks > 4 x 16): gather4160; the second batch for 32 columns (258 chunks > 8 x 16,
    forward; 129 blocks > 8 x 16, backward), the head-partial loop beyond 64 blocks and three wide partials per lane (129
    workgroups): gather16512; the residency limit, 4 x 64 = 256 workgroups with four partials per lane, once as two launches and
    once as one (cdc_tower_step): resident256;
  * fused BCE: int16 labels (rows*_bce), fp32 labels with soft ones (bce_f32, nt4), bce_group NULL (bce_nogroup), -1 and n_tower
    among valid groups (bce_outside, bce_outside16), every row in tower 1 of 3 at M = 257 (bce_one: that tower's workgroups run
    three rounds of 4 x 12 wide rows per block, towers 0 and 2 publish nothing but zero records — the +0 -> -0 path — and must
    come out with EXACTLY zero gradients: the reference's bound there is zero), outputs of exactly 1 / 4e-18 / 0 through
    bo = 40 / -40 / -110 (extreme: both clamps of the loss and the 1e-12 floor);
  * a zero row of W1 with zero bias (z1 column exactly 0, invstd = eps^-1/2), a zero gamma, a zero wo element: degen, degen_dout.

Bit equalities the code implies, asserted with assert_bits_equal: cdc_tower_step against cdc_tower_fwd + cdc_tower_bwd at every
fused-BCE case; the padded against the tight layout; four consecutive launch pairs on one workspace (both record copies, twice)
against a fresh one; tower 0 of a three-tower launch against the same tower launched alone (z, a1h, a2, statistics).

cdc_tower_dp on one device.  One rank, six phases, the exchange buffers left as written (M = 2, 129, 257): every forward tensor
and every gradient is BIT-equal to cdc_tower_fwd / _bwd — the phases run tw_fwd_chunk_sums, tw_gather_sums, tw_block_sums and
the head / wide partial loops in the monolithic order, and (float)sum, 1 / (float)M are formed the same way — except bce_loss:
phase 4 adds a block's rows over ALL towers (tower 0's workgroup), the monolithic backward per (tower, block), so the loss is
held to the float64 bound instead.  Two simulated ranks (shares 128 + 1 and 65 + 64 of 129 rows, dropout off: a rank draws its
mask by LOCAL row): each phase runs for both shares, the four exchange buffers are added on the device in between; results are held
to the float64 reference of the GLOBAL batch, parameter gradients and the loss as the sum of the two ranks' local sums."""
import ctypes as C

import numpy as np
import pytest
import torch

import tower_ref as R
from helpers import OUT_SENTINEL, SUM_FIG, U24, PadBuf, PadBufH, assert_bits_equal, assert_bounded, capped, nan_like

pytestmark = pytest.mark.gpu
CASES = R.cases()
BCE = [c for c in CASES if R.bce(c)]
SMALL = [c for c in CASES if c["M"] <= 300]
XR = 2                                          # sentinel rows below row M of every output matrix
E_BADARG, E_TOOBIG, E_ALIGN = -1, -2, -3
_DATA = {}


@pytest.fixture(scope="module")
def lib(cuda):
    from cdcmdr_amd import _lib as L
    return L.load()


def data(c):
    if c["name"] not in _DATA:
        _DATA[c["name"]] = R.make_data(c)
    return _DATA[c["name"]]


def ids(cs):
    return [c["name"] for c in cs]


class Rows:
    """an fp32 output matrix [M, cols] with XR sentinel rows below it, inside a PadBuf"""

    def __init__(self, dev, init, pad):
        init = np.asarray(init, dtype=np.float32)
        self.M = init.shape[0]
        self.b = PadBuf(dev, np.vstack([init, np.full((XR, init.shape[1]), OUT_SENTINEL, np.float32)]), out=True, pad=pad)
        self.ptr, self.ld = self.b.ptr, self.b.ld

    def read(self, what):
        h = self.b.read(what)
        assert (h[self.M:] == np.float32(OUT_SENTINEL)).all(), f"{what}: rows below M written"
        return h[:self.M]


class Launch:
    """fresh device buffers for a case in layout "t" (tight) or "p" (padded) and the cdc_tower_args over them"""

    def __init__(self, lib, dev, c, D, lay="t", ws=None, dp=False, inv_count=None):
        from cdcmdr_amd import _lib as L
        self.L, self.lib, self.c, self.dev = L, lib, c, dev
        M, n, K, H0 = c["M"], c["n_tower"], c["wide"], c["H0"]
        fp, hp, op = (0, 0, 0) if lay == "t" else (4, 8, 3)
        a = self.a = R.scalar_args(L.TowerArgs(), c)
        if inv_count is not None:
            a.bce_inv_count = inv_count
        self.keep, self.fo, self.bo, self.nbt = [], {}, {}, {}
        k = self._k
        vec = lambda v: k(PadBuf(dev, np.asarray(v, dtype=np.float32).reshape(1, -1)))
        ovec = lambda n_, init=None: k(PadBuf(dev, nan_like(1, n_) if init is None else np.asarray(init, np.float32).reshape(1, -1), out=True))
        nul = set(c["null"])
        if c["step"] is not None and c["p"] > 0:
            a.seed_offset_dev = k(torch.tensor([c["step"]], dtype=torch.int32, device=dev)).data_ptr()
        for t in range(n):
            T = a.t[t]
            xh = k(PadBufH(dev, D["x"][t], pad=hp))
            T.xh, T.ldxh = xh.ptr, xh.ld
            for l, Y, Kin, N in ((1, T.l1, H0, R.H1), (2, T.l2, R.H1, R.H2)):
                W = np.asarray(D[f"W{l}"][t], dtype=np.float32)
                wt = np.zeros((Kin, 64), np.float32)
                wt[:, :N] = W.T
                wh, wtb = k(PadBufH(dev, W, pad=hp)), k(PadBufH(dev, wt, pad=hp))
                Y.wh, Y.ldwh, Y.wt, Y.ldwt = wh.ptr, wh.ld, wtb.ptr, wtb.ld
                Y.bias, Y.gamma, Y.beta = vec(D[f"b{l}"][t]).ptr, vec(D[f"g{l}"][t]).ptr, vec(D[f"be{l}"][t]).ptr
                z = self.fo[f"z{l}_{t}"] = Rows(dev, nan_like(M, N), fp)
                Y.z, Y.ldz = z.ptr, z.ld
                dzh = self.bo[f"dzh{l}_{t}"] = PadBufH(dev, nan_like(M, N), out=True, pad=hp, extra_rows=XR)
                Y.dzh, Y.lddzh = dzh.ptr, dzh.ld
                self.fo[f"mean{l}_{t}"], self.fo[f"inv{l}_{t}"] = ovec(N), ovec(N)
                Y.save_mean, Y.save_invstd = self.fo[f"mean{l}_{t}"].ptr, self.fo[f"inv{l}_{t}"].ptr
                if c["running"]:
                    self.fo[f"rm{l}_{t}"], self.fo[f"rv{l}_{t}"] = ovec(N, D[f"rm{l}"][t]), ovec(N, D[f"rv{l}"][t])
                    Y.running_mean, Y.running_var = self.fo[f"rm{l}_{t}"].ptr, self.fo[f"rv{l}_{t}"].ptr
                if c["nbt"]:
                    self.nbt[f"nbt{l}_{t}"] = torch.tensor([D[f"nbt{l}"][t]], dtype=torch.int64, device=dev)
                    Y.num_batches_tracked = self.nbt[f"nbt{l}_{t}"].data_ptr()
                if "dgamma" not in nul:
                    self.bo[f"dgamma{l}_{t}"] = ovec(N)
                    Y.dgamma = self.bo[f"dgamma{l}_{t}"].ptr
                if "dbeta" not in nul:
                    self.bo[f"dbeta{l}_{t}"] = ovec(N)
                    Y.dbeta = self.bo[f"dbeta{l}_{t}"].ptr
            a1h = self.fo[f"a1h_{t}"] = PadBufH(dev, nan_like(M, R.H1), out=True, pad=hp, extra_rows=XR)
            a2 = self.fo[f"a2_{t}"] = Rows(dev, nan_like(M, R.H2), fp)
            T.a1h, T.lda1h, T.a2, T.lda2 = a1h.ptr, a1h.ld, a2.ptr, a2.ld
            T.wo = vec(D["wo"][t]).ptr
            if D["bo"][t] is not None:
                T.bo = vec(D["bo"][t]).ptr
                if "dbo" not in nul:
                    self.bo[f"dbo_{t}"] = ovec(1)
                    T.dbo = self.bo[f"dbo_{t}"].ptr
            if "dwo" not in nul:
                self.bo[f"dwo_{t}"] = ovec(R.H2)
                T.dwo = self.bo[f"dwo_{t}"].ptr
            if "dx" not in nul:
                dx = self.bo[f"dx_{t}"] = Rows(dev, D["dx0"][t] if c["acc_dx"][t] else nan_like(M, H0), fp)
                T.dx, T.lddx = dx.ptr, dx.ld
            if dp:
                d2, d1 = k(torch.full((M, R.H2), float("nan"), device=dev)), k(torch.full((M, R.H1), float("nan"), device=dev))
                T.dy2, T.lddy2, T.dy1, T.lddy1 = d2.data_ptr(), R.H2, d1.data_ptr(), R.H1
        out = self.fo["out"] = Rows(dev, nan_like(M, n), op)
        a.out, a.ld_out = out.ptr, out.ld
        if K:
            wx = k(PadBuf(dev, D["wx"], pad=fp))
            a.wide_x, a.ld_wide, a.wide_w = wx.ptr, wx.ld, vec(D["ww"]).ptr
            if D["wb"] is not None:
                a.wide_bias = vec(D["wb"]).ptr
                if "wide_dbias" not in nul:
                    self.bo["wide_dbias"] = ovec(1)
                    a.wide_dbias = self.bo["wide_dbias"].ptr
            if "wide_dx" not in nul:
                g = self.bo["wide_dx"] = Rows(dev, D["wdx0"] if c["acc_wide"] else nan_like(M, K), fp)
                a.wide_dx, a.ld_wide_dx = g.ptr, g.ld
            if "wide_dw" not in nul:
                self.bo["wide_dw"] = ovec(K)
                a.wide_dw = self.bo["wide_dw"].ptr
        if R.bce(c):
            y = k(torch.from_numpy(D["y"]).to(dev))
            if D["y"].dtype == np.int16:
                a.bce_y_i16 = y.data_ptr()
            else:
                a.bce_y_f32 = y.data_ptr()
            if D["group"] is not None:
                a.bce_group = k(torch.from_numpy(D["group"]).to(dev)).data_ptr()
            self.bo["loss"] = ovec(1)
            a.bce_loss = self.bo["loss"].ptr
        else:
            do = k(PadBuf(dev, D["dout"], pad=op))
            a.d_out, a.ld_dout = do.ptr, do.ld
        nbytes = int(lib.cdc_tower_workspace_bytes(C.byref(a)))
        assert nbytes > 8192
        if ws is None:
            raw = torch.zeros(nbytes + 128, dtype=torch.uint8, device=dev)
            off = (-raw.data_ptr()) % 128
            ws = raw[off:off + nbytes]
        self.ws = ws
        assert self.ws.numel() >= nbytes and self.ws.data_ptr() % 128 == 0
        self.err = torch.zeros(1, dtype=torch.int32, device=dev)
        a.workspace, a.err = self.ws.data_ptr(), self.err.data_ptr()
        if dp:
            self.ex = [torch.zeros(2 * n * C_ + n, dtype=torch.float64, device=dev) for C_ in (R.H1, R.H2, R.H2, R.H1)]
            for e in range(4):
                a.exchange[e] = self.ex[e].data_ptr()

    def _k(self, b):
        self.keep.append(b)
        return b

    def run(self, name, *extra):
        rc = getattr(self.lib, name)(C.byref(self.a), *extra, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        self.L.check(rc, name)
        torch.cuda.synchronize()
        assert int(self.err.item()) == 0, f"{self.c['name']} {name}{extra}: error word {int(self.err.item()):#x}"
        return self

    def _read(self, bufs):
        out = {}
        for name, b in bufs.items():
            v = b.read(f"{self.c['name']} {name}")
            out[name] = v.reshape(-1) if isinstance(b, PadBuf) else v
        return out

    def forward(self):
        out = self._read(self.fo)
        out.update({name: int(v.item()) for name, v in self.nbt.items()})
        return out

    def backward(self):
        return self._read(self.bo)


def same_bits(a, b, what, skip=()):
    assert a.keys() == b.keys(), (what, a.keys() ^ b.keys())
    for k in a:
        if k in skip:
            continue
        if k.startswith("nbt"):
            assert a[k] == b[k], f"{what} {k}"
        else:
            assert_bits_equal(a[k], b[k], f"{what} {k}")


def two_launches(lib, dev, c, lay="t", ws=None):
    D = data(c)
    A = Launch(lib, dev, c, D, lay, ws)
    A.run("cdc_tower_fwd")
    f = A.forward()
    A.run("cdc_tower_bwd")
    assert_bits_equal(A.fo["out"].read("out"), f["out"], "out after the backward")
    return f, A.backward()


# ------------------------------------------------------------------------------------------------------------------------
# both directions against float64, every case
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CASES, ids=ids(CASES))
def test_forward_and_backward_against_float64(cuda, lib, c):
    D = data(c)
    f, b = two_launches(lib, cuda, c)
    S = R.saved({**f, **b}, c)
    R.compare(f, R.ref_forward(c, D, S), f"{c['name']} fwd")
    want = R.ref_backward(c, D, S)
    R.compare(b, want, f"{c['name']} bwd")
    assert {k for k, v in want.items() if isinstance(v, tuple)} == set(b)
    if c["name"] == "bce_one":                                       # towers 0 and 2: zero records in, exactly zero out
        for t in (0, 2):
            for k in ("dwo", "dbo", "dgamma1", "dgamma2", "dbeta1", "dbeta2", "dx", "dzh1", "dzh2"):
                assert not b[f"{k}_{t}"].any(), f"{k}_{t}"
    if c["name"] == "extreme":
        assert (f["out"][:, 0] == 1).all() and (f["out"][:, 2] == 0).all()
    if c["name"] == "degen":
        assert all((f[f"z1_{t}"][:, 5] == 0).all() and f[f"mean1_{t}"][5] == 0 for t in range(c["n_tower"]))


@pytest.mark.parametrize("c", BCE, ids=ids(BCE))
def test_one_launch_equals_the_two_launches(cuda, lib, c):
    f, b = two_launches(lib, cuda, c)
    A = Launch(lib, cuda, c, data(c)).run("cdc_tower_step")
    same_bits(A.forward(), f, f"{c['name']} step, forward")
    same_bits(A.backward(), b, f"{c['name']} step, backward")


@pytest.mark.parametrize("c", SMALL, ids=ids(SMALL))
def test_padded_layout_gives_the_tight_layouts_bits(cuda, lib, c):
    f, b = two_launches(lib, cuda, c)
    fp, bp = two_launches(lib, cuda, c, "p")
    same_bits(fp, f, f"{c['name']} padded, forward")
    same_bits(bp, b, f"{c['name']} padded, backward")


@pytest.mark.parametrize("name", ["rows257_bce", "rows129_dout", "wide260"])
def test_workspace_reuse_gives_a_fresh_workspaces_bits(cuda, lib, name):
    c = R.by_name(name)
    f, b = two_launches(lib, cuda, c)
    first = Launch(lib, cuda, c, data(c))
    ws = first.ws
    for i in range(4):                                               # record copies 0, 1, 0, 1
        fi, bi = two_launches(lib, cuda, c, ws=ws)
        same_bits(fi, f, f"{name} launch pair {i}, forward")
        same_bits(bi, b, f"{name} launch pair {i}, backward")
    if R.bce(c):
        A = Launch(lib, cuda, c, data(c), ws=ws).run("cdc_tower_step")
        same_bits(A.backward(), b, f"{name} step on the used workspace")


def test_a_tower_does_not_depend_on_its_neighbours(cuda, lib):
    c = R.by_name("rows129_dout")
    D = data(c)
    f, _ = two_launches(lib, cuda, c)
    c1 = dict(c, n_tower=1, acc_dx=c["acc_dx"][:1])
    D1 = {k: (v[:1] if isinstance(v, list) else v) for k, v in D.items()}
    D1["dout"] = D["dout"][:, :1].copy()
    A = Launch(lib, cuda, c1, D1).run("cdc_tower_fwd")
    f1 = A.forward()
    for k in ("z1_0", "a1h_0", "z2_0", "a2_0", "mean1_0", "inv1_0", "mean2_0", "inv2_0", "rm1_0", "rv1_0", "rm2_0", "rv2_0"):
        assert_bits_equal(f1[k], f[k], f"tower 0 alone, {k}")


# ------------------------------------------------------------------------------------------------------------------------
# cdc_tower_dp on one device
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rows2_bce", "rows129_dout", "rows129_bce", "rows257_bce", "h128_257"])
def test_six_phases_on_one_rank_equal_the_two_launches(cuda, lib, name):
    c = R.by_name(name)
    D = data(c)
    f, b = two_launches(lib, cuda, c)
    A = Launch(lib, cuda, c, D, dp=True)
    for phase in range(1, 7):
        A.run("cdc_tower_dp", phase)
    fd, bd = A.forward(), A.backward()
    same_bits(fd, f, f"{name} dp, forward")
    same_bits(bd, b, f"{name} dp, backward", skip=("loss",))
    if R.bce(c):                                                     # another order of the rows' double sum: the float64 bound
        want = R.ref_backward(c, D, R.saved({**fd, **bd}, c))["loss"]
        assert_bounded(bd["loss"], want[0], want[1], f"{name} dp loss")


DP_CASES = [R.case("dp_bce", 129, p=0.0, form="i16"), R.case("dp_dout", 129, p=0.0, acc_dx=(0, 1, 0), acc_wide=1),
            R.case("dp_f32", 129, p=0.0, form="f32", group="outside", relu=0)]


@pytest.mark.parametrize("shares", [(128, 1), (65, 64)], ids=["128+1", "65+64"])
@pytest.mark.parametrize("c", DP_CASES, ids=ids(DP_CASES))
def test_two_simulated_ranks_against_the_global_batch(cuda, lib, c, shares):
    D = data(c)
    n = c["n_tower"]
    ranks, lo = [], 0
    for m in shares:
        rows = slice(lo, lo + m)
        Dk = {k: ([a[rows] if (k in ("x", "dx0")) else a for a in v] if isinstance(v, list) else v) for k, v in D.items()}
        for k in ("wx", "wdx0", "dout", "y", "group"):
            if Dk.get(k) is not None:
                Dk[k] = np.ascontiguousarray(D[k][rows])
        ranks.append(Launch(lib, cuda, dict(c, M=m), Dk, dp=True, inv_count=R.inv_count(c) if R.bce(c) else None))
        lo += m
    for phase in range(1, 7):
        for A in ranks:
            A.run("cdc_tower_dp", phase)
        e = {1: 0, 2: 1, 4: 2, 5: 3}.get(phase)
        if e is not None:                                            # the all-reduce of the exchange buffer
            total = ranks[0].ex[e] + ranks[1].ex[e]
            for A in ranks:
                A.ex[e].copy_(total)
            assert total[-n:].tolist() == [float(c["M"])] * n
    F, Bk = [A.forward() for A in ranks], [A.backward() for A in ranks]
    got, local = {}, {}
    for k in list(F[0]) + list(Bk[0]):
        u, v = (F[0][k], F[1][k]) if k in F[0] else (Bk[0][k], Bk[1][k])
        if k.startswith(("mean", "inv", "rm", "rv", "nbt")):         # every rank keeps the module's statistics of the GLOBAL batch
            if k.startswith("nbt"):
                assert u == v
            else:
                assert_bits_equal(u, v, f"{k} on the two ranks")
            got[k] = u
        elif k.startswith(("dgamma", "dbeta", "dwo", "dbo", "wide_dw", "wide_dbias", "loss")):
            got[k], local[k] = u.astype(np.float64) + v.astype(np.float64), np.abs(u).astype(np.float64) + np.abs(v)
        else:
            got[k] = np.concatenate([u, v], 0)
    S = R.saved(got, c)
    R.compare(got, R.ref_forward(c, D, S), f"{c['name']} {shares} fwd")
    want = R.ref_backward(c, D, S)
    for k, v in want.items():
        if isinstance(v, tuple):
            bound = v[1] if k not in local else capped(v[1] + U24 * local[k], v[0], SUM_FIG)      # each rank rounds its local sum
            assert_bounded(got[k], v[0], bound, f"{c['name']} {shares} bwd {k}")


# ------------------------------------------------------------------------------------------------------------------------
# argument checks: refused without a launch
# ------------------------------------------------------------------------------------------------------------------------
def test_violations_of_the_argument_rules_are_refused(cuda, lib):
    c = R.by_name("rows65_bce")
    D = data(c)

    def tried(fn, rc, change):
        A = Launch(lib, cuda, c, D, "p", dp=True)
        change(A.a)
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        args = (C.byref(A.a), 4, stream) if fn == "cdc_tower_dp" else (C.byref(A.a), stream)
        assert getattr(lib, fn)(*args) == rc, (fn, lib.cdc_last_error())
        torch.cuda.synchronize()
        assert int(A.err.item()) == 0 and np.isnan(A.fo["z1_0"].read("z1")).all() and np.isnan(A.bo["dzh1_0"].read("dzh1")).all()

    def setter(path, value):
        def change(a):
            obj = a
            for p in path[:-1]:
                obj = obj[p] if isinstance(p, int) else getattr(obj, p)
            if isinstance(path[-1], int):
                obj[path[-1]] = value
            else:
                setattr(obj, path[-1], value(getattr(obj, path[-1])) if callable(value) else value)
        return change

    fwd_bad = [(("t", 1, "xh"), lambda p: p + 2), (("t", 2, "l1", "z"), lambda p: p + 4), (("t", 0, "ldxh"), lambda v: v + 4),
               (("wide_K",), 30), (("workspace",), lambda p: p + 64), (("ld_out",), c["n_tower"] - 1), (("t", 1, "l2", "ldwh"), 60),
               (("t", 0, "l2", "ldz"), 34), (("t", 0, "lda1h"), lambda v: v + 4), (("drop_p",), 1.0), (("H0",), 96), (("ld_wide",), 29)]
    for path, value in fwd_bad:
        for fn in ("cdc_tower_fwd", "cdc_tower_step"):
            tried(fn, E_BADARG, setter(path, value))
    tried("cdc_tower_fwd", E_TOOBIG, setter(("M",), 86 * 128))
    for fn in ("cdc_tower_bwd", "cdc_tower_step", "cdc_tower_dp"):
        tried(fn, E_ALIGN, setter(("t", 1, "dx"), lambda p: p + 4))
        tried(fn, E_ALIGN, setter(("t", 0, "lddx"), lambda v: v + 2))
        tried(fn, E_ALIGN, setter(("ld_wide_dx",), lambda v: v + 1))
        tried(fn, E_BADARG, setter(("t", 2, "l1", "dzh"), lambda p: p + 2))
        tried(fn, E_BADARG, setter(("t", 2, "l2", "ldwt"), 56))
        tried(fn, E_BADARG, setter(("bce_loss",), None))
        tried(fn, E_BADARG, setter(("bce_y_i16",), None))            # neither labels nor d_out; tower_step without labels
        tried(fn, E_BADARG, setter(("bce_inv_count",), 0.0))
    tried("cdc_tower_dp", E_BADARG, setter(("t", 1, "dy1"), None))
    tried("cdc_tower_dp", E_BADARG, setter(("exchange", 3), None))
