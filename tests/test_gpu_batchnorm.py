"""The BatchNorm launches (csrc/rowops.hip: cdc_bn_fwd, cdc_bn_bwd) straight through the C-ABI against the float64 restatement of
tests/bn_ref.py — every stride, flag, NULL pointer, row group and phase chosen by the test.

Buffers are padded (helpers.PadBuf, HalfBuf here for bf16): input padding and the rows of other groups are NaN, output padding a
sentinel that must come back bit-unchanged, rows of other groups in an output must stay as they were; accumulate targets start
from random values, plain stores from NaN.  The bounds are derived in bn_ref.py; tests/test_bn_ref_cpu.py shows on the CPU that
they accept an fp32 restatement in the kernels' order and reject nine seeded defects at every shape used here.

The backward is run from the forward's own outputs (y or its bf16 twin, save_mean, save_invstd), as the head's test does."""
import ctypes as C

import numpy as np
import pytest
import torch

import bn_ref as R
from helpers import OUT_SENTINEL, PAD, PadBuf, assert_bits_equal, assert_bounded, nan_like

gpu = pytest.mark.gpu
BADARG = -1
SENT_BITS = int(R.bf16_bits(np.float32(OUT_SENTINEL)).reshape(-1)[0])


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class HalfBuf:
    """PadBuf for a bf16 matrix: values are rounded to bf16, NaN input padding, sentinel output padding."""

    def __init__(self, dev, values, out=False, pad=PAD):
        values = np.asarray(values, dtype=np.float32)
        self.rows, self.cols = values.shape
        self.ld = self.cols + pad
        host = np.full((self.rows, self.ld), SENT_BITS if out else 0x7FC0, dtype=np.uint16)
        host[:, :self.cols] = R.bf16_bits(values)
        self.host0 = host
        self.t = torch.from_numpy(host.view(np.int16).copy()).to(dev)

    @property
    def ptr(self):
        return self.t.data_ptr()

    def read(self, what="buffer"):
        h = self.t.cpu().numpy().view(np.uint16)
        assert np.array_equal(h[:, self.cols:], self.host0[:, self.cols:]), f"{what}: padding written"
        return R.bf16_from_bits(h[:, :self.cols]).reshape(self.rows, self.cols)


def _poisoned(s, i, v):
    """an input of segment i: rows of other groups are NaN"""
    out = np.full((R.launch_rows(s), s["C"][i]), np.nan, np.float32)
    rows = R.seg_rows(s, i)
    out[rows] = np.asarray(v, np.float32)[rows]
    return out


def _group_rows(buf, s, i, what):
    """an output of segment i: the group's rows; every other row must be bit-unchanged"""
    full, rows = buf.read(what), R.seg_rows(s, i)
    other = np.setdiff1d(np.arange(full.shape[0]), rows)
    if other.size:
        start = buf.host0[:, :buf.cols]
        start = R.bf16_from_bits(start).reshape(full.shape) if isinstance(buf, HalfBuf) else start
        assert_bits_equal(full[other], start[other], f"{what}: rows of other groups")
    return full[rows]


class Launch:
    """Fresh padded device buffers for one spec and the two argument blocks over them."""

    def __init__(self, dev, s, D):
        from cdcmdr_amd import _lib as L
        self.L, self.lib, self.s, self.D, self.dev = L, L.load(), s, D, dev
        self.rows, self.keep = R.launch_rows(s), []
        self.n_chunks = max(-(-self.rows // R.ROWS_PER_BLOCK), 1)
        self.ro = None if s["groups"] is None else self._k(torch.tensor(np.concatenate([[0], np.cumsum(s["groups"])]), dtype=torch.int32, device=dev))
        self.step = None if s["step"] is None else self._k(torch.tensor([s["step"]], dtype=torch.int32, device=dev))
        self.ws = self._k(torch.full((2 * self.n_chunks * sum(s["C"]),), float("nan"), dtype=torch.float64, device=dev))
        self.fa = self.ba = None

    def _k(self, b):
        self.keep.append(b)
        return b

    def _buf(self, half, values, out=False, pad=PAD):
        return self._k((HalfBuf if half else PadBuf)(self.dev, values, out=out, pad=pad))

    # ---- forward ----
    def fwd_args(self):
        s, D, L = self.s, self.D, self.L
        a = self.fa = L.BnFwdArgs()
        a.n_seg, a.training, a.relu, a.skip_le1 = len(s["C"]), s["training"], s["relu"], s["skip_le1"]
        a.eps, a.momentum, a.drop_p, a.seed = s["eps"], s["momentum"], s["drop_p"], s["seed"]
        a.seed_offset_dev = None if self.step is None else self.step.data_ptr()
        a.M, a.row_offsets, a.workspace = self.rows, None if self.ro is None else self.ro.data_ptr(), self.ws.data_ptr()
        self.f = []
        for i, Cn in enumerate(s["C"]):
            S, pad, b = a.s[i], s["pad"][i], {}
            b["x"] = self._buf(s["xh"], _poisoned(s, i, D["x"][i]), pad=pad)
            S.x, S.ldx, S.half = b["x"].ptr, b["x"].ld, L.BN_X_BF16 if s["xh"] else 0
            if "f" in s["y"]:
                b["y"] = self._buf(False, nan_like(self.rows, Cn), out=True, pad=pad)
                S.y, S.ldy = b["y"].ptr, b["y"].ld
            if "h" in s["y"]:
                b["yh"] = self._buf(True, nan_like(self.rows, Cn), out=True, pad=pad)
                S.yh, S.ldyh = b["yh"].ptr, b["yh"].ld
            if s["gb"]:
                b["gamma"], b["beta"] = self._buf(False, D["gamma"][i]), self._buf(False, D["beta"][i])
                S.gamma, S.beta = b["gamma"].ptr, b["beta"].ptr
            if s["running"]:
                b["running_mean"], b["running_var"] = self._buf(False, D["rm"][i], out=True), self._buf(False, D["rv"][i], out=True)
                S.running_mean, S.running_var = b["running_mean"].ptr, b["running_var"].ptr
            b["save_mean"], b["save_invstd"] = self._buf(False, nan_like(1, Cn), out=True), self._buf(False, nan_like(1, Cn), out=True)
            S.save_mean, S.save_invstd = b["save_mean"].ptr, b["save_invstd"].ptr
            if s["nbt"]:
                b["nbt"] = self._k(torch.tensor([D["nbt"][i], -5], dtype=torch.int64, device=self.dev))
                S.num_batches_tracked = b["nbt"].data_ptr()
            S.C, S.row_group = Cn, s["seg_group"][i]
            self.f.append(b)
        return a

    def fwd_call(self, phase=0, exchange=None, stats_ready=0):
        a = self.fa or self.fwd_args()
        a.phase, a.exchange, a.stats_ready = phase, None if exchange is None else exchange.data_ptr(), stats_ready
        self.L.check(self.lib.cdc_bn_fwd(C.byref(a), _stream()), "cdc_bn_fwd")

    def fwd_read(self):
        got = []
        for i, b in enumerate(self.f):
            g = {k: _group_rows(b[k], self.s, i, f"{k}{i}") for k in ("y", "yh") if k in b}
            for k in ("save_mean", "save_invstd", "running_mean", "running_var"):
                if k in b:
                    g[k] = b[k].read(f"{k}{i}").reshape(-1)
            if "nbt" in b:
                g["nbt"] = [int(v) for v in b["nbt"].cpu()]
            got.append(g)
        return got

    def forward(self):
        self.fwd_call()
        return self.fwd_read()

    # ---- backward ----
    def bwd_args(self, Y, MEAN, INV):
        s, D, L = self.s, self.D, self.L
        a = self.ba = L.BnBwdArgs()
        a.n_seg, a.training, a.relu, a.eps, a.mask_scale = len(s["C"]), s["training"], s["relu"], s["eps"], R.mask_scale(s)
        a.M, a.row_offsets = self.rows, None if self.ro is None else self.ro.data_ptr()
        self.bws = self._k(torch.full((2 * self.n_chunks * sum(s["C"]),), float("nan"), dtype=torch.float64, device=self.dev))
        a.workspace = self.bws.data_ptr()
        self.b = []
        for i, Cn in enumerate(s["C"]):
            S, pad, b = a.s[i], s["pad"][i], {}
            dy, y, x = (self._buf(h, _poisoned(s, i, v), pad=pad) for h, v in ((s["dyh"], D["dy"][i]), (s["yb"], Y[i]), (s["xh"], D["x"][i])))
            S.dy, S.lddy, S.y, S.ldy, S.x, S.ldx = dy.ptr, dy.ld, y.ptr, y.ld, x.ptr, x.ld
            S.half = (L.BN_X_BF16 if s["xh"] else 0) | (L.BN_Y_BF16 if s["yb"] else 0) | (L.BN_DY_BF16 if s["dyh"] else 0)
            S.accumulate_dx = s["acc"][i]
            if "f" in s["dx"]:
                b["dx"] = self._buf(False, D["dx0"][i] if s["acc"][i] else nan_like(self.rows, Cn), out=True, pad=pad)
                S.dx, S.lddx = b["dx"].ptr, b["dx"].ld
            if "h" in s["dx"]:
                b["dxh"] = self._buf(True, nan_like(self.rows, Cn), out=True, pad=pad)
                S.dxh, S.lddxh = b["dxh"].ptr, b["dxh"].ld
            if s["gb"]:
                S.gamma = self._buf(False, D["gamma"][i]).ptr
            S.save_mean, S.save_invstd = self._buf(False, MEAN[i]).ptr, self._buf(False, INV[i]).ptr
            b["dgamma"], b["dbeta"] = self._buf(False, nan_like(1, Cn), out=True), self._buf(False, nan_like(1, Cn), out=True)
            S.dgamma, S.dbeta = b["dgamma"].ptr, b["dbeta"].ptr
            S.C, S.row_group = Cn, s["seg_group"][i]
            self.b.append(b)
        return a

    def bwd_call(self, phase=0, exchange=None):
        a = self.ba
        a.phase, a.exchange = phase, None if exchange is None else exchange.data_ptr()
        self.L.check(self.lib.cdc_bn_bwd(C.byref(a), _stream()), "cdc_bn_bwd")

    def bwd_read(self):
        got = []
        for i, b in enumerate(self.b):
            g = {k: _group_rows(b[k], self.s, i, f"{k}{i}") for k in ("dx", "dxh") if k in b}
            g["dgamma"], g["dbeta"] = b["dgamma"].read(f"dgamma{i}").reshape(-1), b["dbeta"].read(f"dbeta{i}").reshape(-1)
            got.append(g)
        return got

    def backward(self, Y, MEAN, INV):
        self.bwd_args(Y, MEAN, INV)
        self.bwd_call()
        return self.bwd_read()


def check_forward(s, got, F, what):
    R.compare(got, F, what)
    for i, (g, f) in enumerate(zip(got, F)):
        if s["nbt"]:
            assert g["nbt"] == [f["nbt"], -5], f"{what}: num_batches_tracked{i} {g['nbt']} want {f['nbt']}"
        if f["written"] is False:                                                # a skipped group stores no statistics
            assert np.isnan(g["save_mean"]).all() and np.isnan(g["save_invstd"]).all(), f"{what}: statistics of skipped segment {i}"
        if "y" in g and "yh" in g:
            assert_bits_equal(g["yh"], R.bf16_round(g["y"]), f"{what}: yh{i} is not the rounding of y{i}")
        if "keep" in f:
            # the exact mask: dropped elements are exactly 0, and wherever the undropped value is clearly non-zero the element is
            # kept exactly where the stream's restatement keeps it
            want, bound = f["pre"]
            sure = np.abs(want) > 2 * bound + 1e-30
            for k in ("y", "yh"):
                if k in g:
                    assert not g[k][~f["keep"]].any(), f"{what}: {k}{i} has non-zero dropped elements"
                    assert np.array_equal((g[k] != 0)[sure], f["keep"][sure]), f"{what}: {k}{i} dropout mask differs from the stream"
            assert 0.6 < f["keep"].mean() < 0.9 or f["keep"].size < 64


def saved_from(s, D, got):
    """the backward's operands out of the forward's outputs"""
    Y = []
    for i, g in enumerate(got):
        full = np.full((R.launch_rows(s), s["C"][i]), np.nan, np.float32)
        full[R.seg_rows(s, i)] = g["y"] if "y" in g else g["yh"]
        Y.append(full)
    if not s["training"]:
        return (Y,) + R.eval_saved(s, D)
    return Y, [g["save_mean"] for g in got], [g["save_invstd"] for g in got]


def check_backward(s, got, B, what):
    R.compare(got, B, what)
    for i, g in enumerate(got):
        if "dx" in g and "dxh" in g:
            assert_bits_equal(g["dxh"], R.bf16_round(g["dx"]), f"{what}: dxh{i} is not the rounding of dx{i}")


def run_case(dev, s):
    what = f"bn {s['name']} M={s['M']}"
    D = R.make_data(s)
    la = Launch(dev, s, D)
    got = la.forward()
    check_forward(s, got, R.ref_forward(s, D), what + " fwd")
    Y, MEAN, INV = saved_from(s, D, got)
    check_backward(s, la.backward(Y, MEAN, INV), R.ref_backward(s, D, Y, MEAN, INV), what + " bwd")
    return got


# ------------------------------------------------------------------------------------------------------------------------
# column and row geometry
# ------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("pad,Cn", [(3, c) for c in R.ONE_C] + [(4, c) for c in R.V4_C])
def test_bn_geometry(cuda, pad, Cn):
    """One segment: pad 3 forces one column per lane (C = 1, 3, 64, 70); 16-byte aligned rows with C % 4 == 0 take the 16-byte
    lanes, LS = 3..6 each with a full tile and a partial second one; M = 1 (skipped), 2, around one chunk, 3 and 5 chunks, and 10
    chunks (577: more chunks than waves, and than the 8 threads per column of LS = 3)."""
    specs = [s for s in R.geometry_specs() if s["C"] == (Cn,) and s["pad"] == (pad,)]
    assert [s["M"] for s in specs] == list(R.ROWS) and R.family(specs[0]) == ("one" if pad == 3 else "v4")
    for s in specs:
        run_case(cuda, s)


@gpu
@pytest.mark.parametrize("name", ["mixed", "fallbackC", "fallbackLd", "maxseg"])
def test_bn_launch_shapes(cuda, name):
    """mixed: C = 8 beside C = 256, LS = 6 for both (the small segment uses two lanes of a row).  fallbackC / fallbackLd: one
    segment with C % 4 != 0, resp. with unaligned rows, among aligned ones: the launch takes one column per lane throughout.
    maxseg: CDC_MAX_BN_SEGS segments."""
    s = [t for t in R.geometry_specs() if t["name"] == name][0]
    assert R.family(s) == ("one" if name.startswith("fallback") else "v4")
    assert name != "maxseg" or len(s["C"]) == 24
    run_case(cuda, s)


@gpu
@pytest.mark.parametrize("k", range(4))
def test_bn_row_groups(cuda, k):
    """row_offsets with group sizes {0, 1, 2, 64, 65, 130} in shuffled order, segments mapped to groups non-monotonically, two
    segments on one group, skip_le1 0 and 1, both dispatches.  Rows of other groups stay untouched (Launch reads every output
    through _group_rows).  The empty group is the reference's absent domain: under MDR_BatchNorm (skip_le1 = 0) the batch is
    counted and the running statistics stay, under the DNN's rule (skip_le1 = 1) nothing changes at all."""
    s = R.group_specs()[k]
    got = run_case(cuda, s)
    D = R.make_data(s)
    empty = [i for i in range(len(s["C"])) if R.seg_rows(s, i).size == 0]
    assert empty
    for i in empty:
        assert got[i]["nbt"][0] == D["nbt"][i] + (0 if s["skip_le1"] else 1)
        assert_bits_equal(got[i]["running_mean"], D["rm"][i], "running_mean of an empty group")
        assert_bits_equal(got[i]["running_var"], D["rv"][i], "running_var of an empty group")


@gpu
@pytest.mark.parametrize("k", range(len(R.flag_specs())))
def test_bn_flags(cuda, k):
    """The table of bn_ref.flag_specs: training x relu x dropout (p = 0.25, NULL and two values of the device seed offset, the
    exact mask of either stream), NULL gamma / beta / running stats / num_batches_tracked, y / yh / both, dx / dxh / both,
    accumulate_dx, the three bf16 operand flags, a constant column, |mean| / std = 10^3, one-row launches."""
    run_case(cuda, R.flag_specs()[k])


# ------------------------------------------------------------------------------------------------------------------------
# data-parallel phases on one device
# ------------------------------------------------------------------------------------------------------------------------
def _rank_data(u, Du, ranks, parts, k):
    rk = ranks[k]
    D = {key: list(Du[key]) for key in ("gamma", "beta", "rm", "rv", "nbt")}
    for key in ("x", "dy", "dx0"):
        D[key] = []
        for i, Cn in enumerate(u["C"]):
            v = np.full((R.launch_rows(rk), Cn), np.nan, np.float32)
            v[R.seg_rows(rk, i)] = Du[key][i][R.dp_rank_rows(u, ranks, parts, k, i)]
            D[key].append(v)
    return D


def _all_reduce(ex):
    tot = ex[0] + ex[1]
    for e in ex:
        e.copy_(tot)


@gpu
@pytest.mark.parametrize("pad", [3, 4])
@pytest.mark.parametrize("name", list(R.DP_SPLITS))
def test_bn_data_parallel_phases(cuda, name, pad):
    """Two ranks = two argument blocks over disjoint rows, each with its own workspace and exchange buffer: phase 1 on both, the
    exchange buffers added and copied back (the all-reduce), phase 2 on both — against float64 over the union of the rows;
    dgamma / dbeta are local sums, and the two ranks' values together are the union's.  "1+5": a rank holding ONE row of a group
    whose global count is six must still contribute its row to the exchanged backward sums."""
    u, ranks, parts = R.dp_specs(name, pad)
    Du = R.make_data(u)
    n_ex = 2 * sum(u["C"]) + len(u["C"])
    las = [Launch(cuda, rk, _rank_data(u, Du, ranks, parts, k)) for k, rk in enumerate(ranks)]
    ex = [torch.full((n_ex,), float("nan"), dtype=torch.float64, device=cuda) for _ in las]
    for la, e in zip(las, ex):
        la.fwd_call(1, e)
    counts = [e[2 * sum(u["C"]):].cpu().tolist() for e in ex]
    assert counts == [[float(R.seg_rows(rk, i).size) for i in range(len(u["C"]))] for rk in ranks]
    _all_reduce(ex)
    for la, e in zip(las, ex):
        la.fwd_call(2, e)
    F = R.ref_forward(u, Du, n_ranks=2)
    sub = lambda W, k, keys: [{n: ((v[0][parts[i][k]], v[1][parts[i][k]]) if n in keys else v) for n, v in w.items()} for i, w in enumerate(W)]
    gots = [la.fwd_read() for la in las]
    for k, got in enumerate(gots):
        check_forward(u, got, sub(F, k, ("y",)), f"bn dp {name} rank {k} fwd")
    # the backward's operands: the union's y in the union's row order; both ranks hold the same saved statistics
    Y = []
    for i, Cn in enumerate(u["C"]):
        full = np.full((R.launch_rows(u), Cn), np.nan, np.float32)
        for k in range(2):
            full[R.dp_rank_rows(u, ranks, parts, k, i)] = gots[k][i]["y"]
        Y.append(full)
    for key in ("save_mean", "save_invstd"):
        for i in range(len(u["C"])):
            assert_bits_equal(gots[0][i][key], gots[1][i][key], f"{key}{i} of the two ranks")
    MEAN, INV = [g["save_mean"] for g in gots[0]], [g["save_invstd"] for g in gots[0]]
    B = R.ref_backward(u, Du, Y, MEAN, INV, parts=parts)
    ex = [torch.full((n_ex,), float("nan"), dtype=torch.float64, device=cuda) for _ in las]
    for k, (la, e) in enumerate(zip(las, ex)):
        la.bwd_args(saved_from(ranks[k], None, gots[k])[0], MEAN, INV)
        la.bwd_call(1, e)
    _all_reduce(ex)
    backs = []
    for k, (la, e) in enumerate(zip(las, ex)):
        la.bwd_call(2, e)
        got = la.bwd_read()
        want = [{"dx": (b["dx"][0][parts[i][k]], b["dx"][1][parts[i][k]]), "dgamma": b[f"dgamma_r{k}"], "dbeta": b[f"dbeta_r{k}"]}
                for i, b in enumerate(B)]
        check_backward(u, got, want, f"bn dp {name} rank {k} bwd")
        backs.append(got)
    U = R.ref_backward(u, Du, Y, MEAN, INV)
    for i, (b, w) in enumerate(zip(B, U)):
        for key in ("dgamma", "dbeta"):
            assert_bounded(backs[0][i][key].astype(np.float64) + backs[1][i][key], w[key][0], b[f"{key}_r0"][1] + b[f"{key}_r1"][1] + 1e-300,
                           f"bn dp {name} {key}{i}: the two ranks together")


@gpu
def test_bn_phase1_without_rows_returns_zero(cuda):
    """A launch with M = 0 returns 0 and launches nothing; in phase 1 the exchange buffer keeps what it held.  include/cdcmdr.h
    states that callers never do this: every rank's launch covers its local batch (dist.py: the global batch is world_size x the
    local batch, plan.B >= 1 rows on every rank); only a row GROUP can be empty on a rank, and test_bn_data_parallel_phases
    ("0+5") holds that its sums and count are then written as zeros."""
    s = R.spec("norows", (6, 8), 1)
    la = Launch(cuda, s, R.make_data(s))
    ex = torch.full((2 * 14 + 2,), 12345.0, dtype=torch.float64, device=cuda)
    la.fwd_args().M = 0
    la.fwd_call(1, ex)
    assert bool((ex == 12345.0).all())
    la.bwd_args([nan_like(1, c) for c in s["C"]], [nan_like(1, c) for c in s["C"]], [nan_like(1, c) for c in s["C"]]).M = 0
    la.bwd_call(1, ex)
    assert bool((ex == 12345.0).all())
    assert np.isnan(la.fwd_read()[0]["y"]).all()


# ------------------------------------------------------------------------------------------------------------------------
# statistics from the GEMM epilogues (stats_ready)
# ------------------------------------------------------------------------------------------------------------------------
def _r64(n):
    return (n + 63) // 64 * 64


def _shadow(t, pad_rows=True):
    """zero-padded bf16 copy [rows64, cols64 + 64] of an fp32 matrix, as plan.py allocates shadows"""
    rows, cols = t.shape
    sh = torch.zeros((_r64(rows) if pad_rows else rows, _r64(cols) + 64), dtype=torch.bfloat16, device=t.device)
    sh[:rows, :cols] = t.to(torch.bfloat16)
    return sh


def _produce(la, producer, M, Ns, K, with_bias, seed):
    """x of every BatchNorm segment = the output of one linear group of ONE producing launch, whose epilogue writes the
    statistics' partial sums into the BatchNorm launch's workspace.  Returns the call's return code."""
    L, lib, dev = la.L, la.lib, la.dev
    gen = torch.Generator().manual_seed(seed)
    total_c, col0 = sum(Ns), 0
    a = L.G2Args() if producer == "g2" else L.LinFwdArgs()
    if producer == "g2":
        a.n_out = a.n_seg = len(Ns)
        a.mode, a.relu, a.drop_p, a.mask_scale = 0, 0, 0.0, 1.0
    else:
        a.n_groups, a.relu, a.drop_p = len(Ns), 0, 0.0
    for i, N in enumerate(Ns):
        x = la._k((torch.randn(M, K, generator=gen) * 2 + 1).to(dev))
        w = la._k((torch.randn(N, K, generator=gen) / K ** 0.5).to(dev))
        b = la._k(torch.randn(N, generator=gen).to(dev)) if with_bias[i] else None
        y = la.f[i]["x"]                                                         # the BatchNorm segment's (padded) input buffer
        if producer == "g2":
            xh, wh = la._k(_shadow(x)), la._k(_shadow(w, pad_rows=False))
            O, S = a.o[i], a.s[i]
            O.y, O.ldy, O.bias, O.M, O.N, O.act_cols = y.ptr, y.ld, None if b is None else b.data_ptr(), M, N, 0
            O.bn_partial, O.bn_col0, O.bn_total_c, O.stream_id = la.ws.data_ptr(), col0, total_c, i
            S.a, S.lda, S.b, S.ldb, S.Kr, S.out = xh.data_ptr(), xh.stride(0), wh.data_ptr(), wh.stride(0), _r64(K), i
        else:
            G = a.g[i]
            G.x, G.ldx, G.w, G.ldw, G.bias = x.data_ptr(), x.stride(0), w.data_ptr(), w.stride(0), None if b is None else b.data_ptr()
            G.y, G.ldy, G.M, G.N, G.K, G.act_cols = y.ptr, y.ld, M, N, K, 0
            G.bn_partial, G.bn_col0, G.bn_total_c = la.ws.data_ptr(), col0, total_c
        col0 += N
    la.producer_args = a
    if producer == "g2":
        return lambda: lib.cdc_gemm_bf16_nt(C.byref(a), _stream())
    return lambda: lib.cdc_glinear_fwd(C.byref(a), L.PREC_F32 if producer == "f32" else L.PREC_BF16, _stream())


@gpu
@pytest.mark.parametrize("Ns,pad", [((8, 64), 4), ((70, 129), 3)])
@pytest.mark.parametrize("producer", ["f32", "bf16", "g2"])
def test_bn_fused_statistics(cuda, producer, Ns, pad):
    """cdc_glinear_fwd (F32, BF16) and cdc_gemm_bf16_nt (mode 0) write two groups' partial sums into one BatchNorm workspace (one
    column total; group 0 with a bias, group 1 without); cdc_bn_fwd with stats_ready = 1 must then meet the same bounds against
    float64 statistics of the x the GEMM actually wrote."""
    for M in (1, 63, 65, 130, 257):
        s = R.spec(f"fused{producer}", Ns, M, pad=pad)
        D = R.make_data(s)
        la = Launch(cuda, s, D)
        la.fwd_args()
        for b in la.f:                                                           # x is an OUTPUT of the producer: NaN, sentinel padding
            b["x"] = la._buf(False, nan_like(M, b["x"].cols), out=True, pad=pad)
        for i, b in enumerate(la.f):
            la.fa.s[i].x, la.fa.s[i].ldx = b["x"].ptr, b["x"].ld
        call = _produce(la, producer, M, Ns, 40, (True, False), M)
        la.L.check(call(), "producer")
        D["x"] = [b["x"].read(f"x{i}") for i, b in enumerate(la.f)]
        assert all(np.isfinite(x).all() for x in D["x"])
        la.fwd_call(stats_ready=1)
        check_forward(s, la.fwd_read(), R.ref_forward(s, D), f"bn fused {producer} {Ns} M={M}")


@gpu
def test_bn_fused_statistics_argument_checks(cuda):
    s = R.spec("fusedargs", (8, 64), 65, pad=4)
    for producer, text in (("f32", b"cannot feed BatchNorm partial sums"), ("g2", b"cannot feed BatchNorm partial sums")):
        for how in ("act_cols", "row_offsets"):
            if producer == "g2" and how == "row_offsets":
                continue                                                         # (cdc_g2_args has no ragged rows)
            la = Launch(cuda, s, R.make_data(s))
            la.fwd_args()
            call = _produce(la, producer, 65, s["C"], 40, (True, False), 1)
            if how == "act_cols":
                (la.producer_args.o if producer == "g2" else la.producer_args.g)[1].act_cols = 4
            else:
                la.producer_args.row_offsets = la._k(torch.tensor([0, 65, 65], dtype=torch.int32, device=cuda)).data_ptr()
            assert call() == BADARG and text in la.lib.cdc_last_error(), la.lib.cdc_last_error()
            torch.cuda.synchronize()
            assert bool(torch.isnan(la.ws).all()), "a refused launch wrote partial sums"


# ------------------------------------------------------------------------------------------------------------------------
# argument checks
# ------------------------------------------------------------------------------------------------------------------------
@gpu
def test_bn_argument_checks(cuda):
    """Nothing is launched: return code, cdc_last_error(), outputs untouched."""
    s = R.spec("args", (6, 8), 5, y="fh", dx="fh")
    D = R.make_data(s)
    ex = torch.zeros(2 * 14 + 2, dtype=torch.float64, device=cuda)
    Y, MEAN, INV = [nan_like(5, c) for c in s["C"]], [nan_like(1, c) for c in s["C"]], [nan_like(1, c) for c in s["C"]]

    def refused(backward, change, text):
        la = Launch(cuda, s, D)
        a = la.bwd_args(Y, MEAN, INV) if backward else la.fwd_args()
        change(a, la)
        fn = la.lib.cdc_bn_bwd if backward else la.lib.cdc_bn_fwd
        assert fn(C.byref(a), _stream()) == BADARG
        assert text in la.lib.cdc_last_error(), la.lib.cdc_last_error()
        torch.cuda.synchronize()
        out = la.bwd_read() if backward else la.fwd_read()
        assert all(np.isnan(g["dx" if backward else "y"]).all() for g in out), "a refused launch stored results"

    def setter(**kw):
        def change(a, la):
            for k, v in kw.items():
                setattr(a, k, v)
        return change

    def seg_setter(i, **kw):
        def change(a, la):
            for k, v in kw.items():
                setattr(a.s[i], k, v)
        return change

    for n in (0, 25):
        refused(False, setter(n_seg=n), b"bn_fwd: bad argument")
        refused(True, setter(n_seg=n), b"bn_bwd: bad argument")
    refused(False, setter(workspace=None), b"bn_fwd: training needs a workspace")
    refused(True, setter(workspace=None), b"bn_bwd: bad argument")
    refused(False, lambda a, la: (setattr(a, "training", 0), setattr(a.s[1], "running_var", None)), b"bn_fwd: eval needs running stats")
    refused(False, seg_setter(1, ldx=7), b"bn_fwd: segment 1 malformed")
    refused(False, seg_setter(0, half=2), b"bn_fwd: segment 0 malformed")            # CDC_BN_Y_BF16: not a forward operand
    for backward, nm in ((False, b"bn_fwd"), (True, b"bn_bwd")):
        refused(backward, setter(phase=1), nm + b": phases 1/2 need training mode and an exchange buffer")
        refused(backward, setter(phase=2), nm + b": phases 1/2 need training mode and an exchange buffer")
        refused(backward, setter(phase=1, training=0, exchange=ex.data_ptr()), nm + b": phases 1/2 need training mode and an exchange buffer")
        refused(backward, setter(phase=3, exchange=ex.data_ptr()), nm + b": phases 1/2 need training mode and an exchange buffer")
    refused(True, seg_setter(1, dx=None, accumulate_dx=1), b"bn_bwd: segment 1 malformed")
    assert not ex.any()
