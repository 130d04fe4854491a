"""tests/interaction_ref.py (the float64 references of the attention, FM and row-dot GPU tests) against torch float64 autograd on
tiny shapes, the attention's keep mask against a scalar restatement of cdc_uniform, and the references' bounds against seeded
defects.  No GPU."""
import numpy as np
import pytest
import torch

import interaction_ref as I
import weighted_ref as W

RT = 1e-12


def _close(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, f"{what}: shape {got.shape} vs {want.shape}"
    assert np.all(np.abs(got - want) <= RT * (1.0 + np.abs(want))), f"{what}: {np.abs(got - want).max():.3e}"


@pytest.mark.parametrize("B,F,A,H,p", [(1, 1, 4, 1, 0.0), (2, 3, 8, 2, 0.0), (2, 5, 16, 2, 0.5), (3, 4, 12, 3, 0.25)])
def test_attention_reference_matches_torch_float64(B, F, A, H, p):
    rng = np.random.default_rng(B * 100 + F)
    dh = A // H
    qkv32, dout32 = rng.standard_normal((B * F, 3 * A)).astype(np.float32), rng.standard_normal((B * F, A)).astype(np.float32)
    keep = rng.random((B, H, F, F)) >= p                                     # an explicit mask
    t = torch.from_numpy(qkv32).double().requires_grad_(True)
    q, k, v = [x.reshape(B, F, H, dh).transpose(1, 2) for x in t.split(A, dim=1)]
    pr = torch.softmax((q * dh ** -0.5) @ k.transpose(-1, -2), dim=-1)
    pd = pr * torch.from_numpy(keep).double() / (1.0 - p)
    out = (pd @ v).transpose(1, 2).reshape(B * F, A)
    out.backward(torch.from_numpy(dout32).double())
    f = I.attn_forward(qkv32, B, F, A, H, keep, p)
    _close(f["probs"][0], pr.detach().numpy(), "probs")
    _close(f["out"][0], out.detach().numpy(), "out")
    b = I.attn_backward(qkv32, f["probs"][0], dout32, B, F, A, H, keep, p)
    g = t.grad.numpy()
    for i, nm in enumerate(("dq", "dk", "dv")):
        _close(b[nm][0], g[:, i * A:(i + 1) * A], nm)
        assert (b[nm][1] >= 0).all() and np.isfinite(b[nm][1]).all()
    # the bounds: positive wherever a value is not exactly representable, and never above the suite's figures
    assert (f["out"][1] <= I.OUT_FIG[1] + I.OUT_FIG[0] * np.abs(f["out"][0])).all()
    assert (b["dq"][1] <= I.DQKV_FIG[1] + I.DQKV_FIG[0] * np.abs(b["dq"][0])).all()
    # fp32 arithmetic in another order stays inside them; a dropped key does not
    s32 = np.einsum("bhid,bhjd->bhij", (I.f32(qkv32[:, :A]) * np.float32(dh ** -0.5)).reshape(B, F, H, dh).transpose(0, 2, 1, 3),
                    qkv32[:, A:2 * A].reshape(B, F, H, dh).transpose(0, 2, 1, 3)).astype(np.float32)
    e32 = np.exp(s32 - s32.max(-1, keepdims=True))
    p32 = (e32 / e32.sum(-1, keepdims=True, dtype=np.float32)).astype(np.float32)
    assert (np.abs(p32 - f["probs"][0]) <= f["probs"][1]).all()
    if F > 1:
        bad = p32.copy()
        bad[..., -1] = 0
        assert not (np.abs(bad - f["probs"][0]) <= f["probs"][1]).all()


def test_attention_keep_mask_against_scalar_restatement():
    M64 = (1 << 64) - 1

    def uniform(seed, idx):
        z = (seed + idx * 0x9E3779B97F4A7C15) & M64
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        z ^= z >> 31
        return np.float32(z >> 40) * np.float32(1.0 / 16777216.0)

    seed, B, H, F, p = 0x1234_5678_9ABC_DEF1, 5, 3, 26, 0.5
    for step in (None, 0, 3, 70000, -1):
        sd = seed if step is None else (seed + (step & 0xFFFFFFFF) * I.MUL) & M64
        keep = I.attn_keep_mask(seed, step, B, H, F, p)
        assert keep.shape == (B, H, F, F)
        for pair, i, j in ((0, 0, 0), (0, 0, 1), (1, 25, 24), (7, 3, 9), (14, 25, 25), (9, 12, 0)):
            want = not (uniform(sd, (pair * F + i) * F + j) < np.float32(p))
            assert keep[pair // H, pair % H, i, j] == want, (step, pair, i, j)
    assert np.array_equal(I.attn_keep_mask(seed, None, B, H, F, p), I.attn_keep_mask(seed, 0, B, H, F, p))
    assert not np.array_equal(I.attn_keep_mask(seed, 3, B, H, F, p), I.attn_keep_mask(seed, 4, B, H, F, p))
    assert abs(I.attn_keep_mask(seed, 3, 8, 4, 64, p).mean() - 0.5) < 0.01
    assert I.attn_keep_mask(seed, 3, B, H, F, 0.0).all()


@pytest.mark.parametrize("B,F,D", [(1, 1, 1), (3, 2, 5), (4, 5, 3)])
def test_fm_reference_matches_torch_float64(B, F, D):
    rng = np.random.default_rng(B + F + D)
    e32, g32, old32 = (rng.standard_normal(s).astype(np.float32) for s in ((B, F * D), (B,), (B, F * D)))
    t = torch.from_numpy(e32).double().reshape(B, F, D).requires_grad_(True)
    out = 0.5 * (t.sum(1) ** 2 - (t ** 2).sum(1)).sum(1)
    out.backward(torch.from_numpy(g32).double())
    want, bound = I.fm_forward(e32, F, D)
    _close(want, out.detach().numpy(), "fm out")
    assert (bound > 0).all() or F == 1
    g, bg = I.fm_backward(e32, g32, F, D)
    _close(g, t.grad.reshape(B, F * D).numpy(), "fm de")
    g2, _ = I.fm_backward(e32, g32, F, D, old32)
    _close(g2, t.grad.reshape(B, F * D).numpy() + old32.astype(np.float64), "fm de +=")
    if F == 1:
        assert not want.any() and not g.any()                                  # one field: no pair, and the bound is not 0
        assert (bound > 0).all()
    # fp32 in the kernel's order is inside the bound; the field sum without its last field is not
    x = e32.reshape(B, F, D)
    s32, q32 = np.zeros((B, D), np.float32), np.zeros((B, D), np.float32)
    for f in range(F):
        s32, q32 = s32 + x[:, f], q32 + x[:, f] * x[:, f]
    o32 = np.float32(0.5) * (s32 * s32 - q32).sum(1, dtype=np.float32)
    assert (np.abs(o32 - want) <= bound).all()
    if F > 1:
        sb = s32 - x[:, F - 1]
        assert not (np.abs(np.float32(0.5) * (sb * sb - q32).sum(1, dtype=np.float32) - want) <= bound).all()


@pytest.mark.parametrize("sigmoid", [0, 1])
@pytest.mark.parametrize("M,K,n_add,bias", [(1, 1, 0, None), (5, 7, 2, 0.3), (9, 70, 4, -1.5)])
def test_rowdot_reference_matches_torch_float64(M, K, n_add, bias, sigmoid):
    rng = np.random.default_rng(M * 10 + K + sigmoid)
    x32, w32, dout32, old32 = (rng.standard_normal(s).astype(np.float32) for s in ((M, K), (K,), (M,), (M, K)))
    ads = [rng.standard_normal(M).astype(np.float32) for _ in range(n_add)]
    x, w = torch.from_numpy(x32).double().requires_grad_(True), torch.from_numpy(w32).double().requires_grad_(True)
    b = torch.tensor(0.0 if bias is None else float(np.float32(bias)), dtype=torch.float64, requires_grad=True)
    z = x @ w + b
    for a in ads:
        z = z + torch.from_numpy(a).double()
    z.retain_grad()
    out = torch.sigmoid(z) if sigmoid else z
    out.backward(torch.from_numpy(dout32).double())
    f = I.rowdot_forward(x32, w32, None if bias is None else np.float32(bias), ads, sigmoid)
    _close(f["logit"][0], z.detach().numpy(), "logit")
    _close(f["out"][0], out.detach().numpy(), "out")
    g = I.rowdot_backward(x32, w32, dout32, out.detach().numpy(), sigmoid)         # (float64 outputs: the identity itself)
    _close(g["dlogit"][0][:, 0], z.grad.numpy(), "dlogit")
    _close(g["dx"][0], x.grad.numpy(), "dx")
    _close(g["dw"][0][0], w.grad.numpy(), "dw")
    _close(g["dbias"][0][0, 0], b.grad.numpy(), "dbias")
    g2 = I.rowdot_backward(x32, w32, dout32, out.detach().numpy(), sigmoid, old32)
    _close(g2["dx"][0], x.grad.numpy() + old32.astype(np.float64), "dx +=")
    if not sigmoid:
        assert not g["dlogit"][1].any()                                       # a copy: exact
    # an fp32 evaluation is inside the forward bound, one without its last column is not
    z32 = (x32 * w32[None, :]).sum(1, dtype=np.float32) + np.float32(0 if bias is None else bias)
    for a in ads:
        z32 = z32 + a
    o32 = I._sig32(z32) if sigmoid else z32
    assert (np.abs(o32 - f["out"][0]) <= f["out"][1]).all()
    if K > 1:
        zb = z32 - x32[:, -1] * w32[-1]
        ob = I._sig32(zb) if sigmoid else zb
        assert not (np.abs(ob - f["out"][0]) <= f["out"][1]).all()


def test_unweighted_fused_bce_reference_is_the_weighted_one_with_ones():
    """weighted_ref.head_backward(w = None), which tests/test_gpu_rowdot.py uses for the fused BCE: the values of all-ones weights,
    bounds one rounding tighter, and torch's float64 BCE on the own column."""
    rng = np.random.default_rng(5)
    M, K = 9, (3, 5)
    D = {"x": [rng.standard_normal((M, k)).astype(np.float32) for k in K], "w": [rng.standard_normal(k).astype(np.float32) for k in K],
         "y": rng.integers(0, 2, size=M).astype(np.int16), "group": np.array([0, 1, -1, 2, 1, 0, 1, 1, 0], dtype=np.int64)}
    out32 = rng.uniform(0.05, 0.95, size=(M, 2)).astype(np.float32)
    a, b = W.head_backward(K, 0, 0, D, out32, None, 1.0 / M), W.head_backward(K, 0, 0, D, out32, np.ones(M, np.float32), 1.0 / M)
    assert set(a) == set(b)
    for k in a:
        _close(a[k][0], b[k][0], k)
        assert (a[k][1] <= b[k][1]).all()
    own = np.where((D["group"] < 0) | (D["group"] >= 2), 0, D["group"])
    o = torch.from_numpy(out32).double().requires_grad_(True)
    loss = torch.nn.functional.binary_cross_entropy(o[torch.arange(M), torch.from_numpy(own)], torch.from_numpy(D["y"]).double())
    loss.backward()
    _close(a["loss"][0][0], float(loss.detach()), "loss")
    d = (o.grad * o.detach() * (1 - o.detach())).numpy()
    for t in range(2):
        _close(a[f"dbias{t}"][0][0, 0], d[:, t].sum(), f"dbias{t}")
        _close(a[f"dw{t}"][0][0], d[:, t] @ D["x"][t].astype(np.float64), f"dw{t}")
