"""The one-launch row sort of 1025 .. 4096 rows (k_sort_dedupe_radix: one workgroup per field, radix passes in LDS).

Integer work, so everything is compared bit for bit with numpy on the host: a stable argsort of the rows as unsigned 32-bit
numbers per field, and the unique rows, segment starts and counts that follow from it.  Only the defined ranges are compared:
uniq_row[f, :cnt], seg_start[f, :cnt + 1], perm[f, :B], uniq_cnt[f].
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = [1025, 2048, 3000, 4096]          # 1025: first size of the radix path; 3000: not a power of two; 4096: its last size


def _oracle(rows_u32):
    """rows_u32 [B, F] uint32 -> per field (perm, uniq, seg_start incl. the closing B)."""
    B, F = rows_u32.shape
    out = []
    for f in range(F):
        order = np.argsort(rows_u32[:, f], kind="stable")
        uniq, starts = np.unique(rows_u32[order, f], return_index=True)
        out.append((order.astype(np.int32), uniq.astype(np.uint32).view(np.int32), np.append(starts, B).astype(np.int32)))
    return out


def _buffers(B, F, dev):
    return (torch.full((F, B), -7, dtype=torch.int32, device=dev), torch.full((F, B + 1), -7, dtype=torch.int32, device=dev),
            torch.full((F, B), -7, dtype=torch.int32, device=dev), torch.full((F,), -7, dtype=torch.int32, device=dev))


def _check(bufs, want, B):
    uniq, seg, perm, cnt = (t.cpu().numpy() for t in bufs)
    for f, (w_perm, w_uniq, w_seg) in enumerate(want):
        n = len(w_uniq)
        assert cnt[f] == n, f"field {f}: {cnt[f]} unique rows, expected {n}"
        assert np.array_equal(perm[f, :B], w_perm), f"field {f}: perm"
        assert np.array_equal(uniq[f, :n], w_uniq), f"field {f}: uniq_row"
        assert np.array_equal(seg[f, :n + 1], w_seg), f"field {f}: seg_start"


def _pattern(name, B, F, rng):
    cols = []
    for f in range(F):
        if name == "all_equal":
            c = np.full(B, 123457 + f, dtype=np.int64)
        elif name == "descending":
            c = np.arange(B, 0, -1, dtype=np.int64) * 3 + 5000 * f
        elif name == "alternating":
            c = np.where(np.arange(B) % 2 == 0, 70000 + f, 9 + f).astype(np.int64)
        elif name == "random_dups":                      # B draws from 1.4 B values: 1 - 1.4 (1 - exp(-1 / 1.4)) = 29 % are repeats
            c = rng.integers(0, int(1.4 * B), size=B) + (1 << 20) * f
        elif name == "high_bits":                        # all four digits differ: every pass runs; values up to 2^31 - 2
            c = np.concatenate([rng.integers(0, 300, size=B // 4), (1 << 24) + rng.integers(-40, 40, size=B // 4),
                                (1 << 31) - 2 - rng.integers(0, 3, size=B // 4)])
            c = np.concatenate([c, rng.integers(0, 1 << 31, size=B - len(c))])
            c = rng.permutation(c)
        else:
            raise AssertionError(name)
        cols.append(c)
    return np.stack(cols, axis=1).astype(np.int32)


def _sort(lib, L, d_idx, bufs, B, F, scratch=None):
    uniq, seg, perm, cnt = bufs
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    L.check(lib.cdc_embed_sort_dedupe(d_idx.data_ptr(), uniq.data_ptr(), seg.data_ptr(), perm.data_ptr(), cnt.data_ptr(),
                                      None if scratch is None else scratch.data_ptr(), B, F, s), "sort")


@pytest.mark.parametrize("pattern", ["all_equal", "descending", "alternating", "random_dups", "high_bits"])
@pytest.mark.parametrize("F", [1, 3])
@pytest.mark.parametrize("B", SIZES)
def test_radix_sort_key_patterns(cuda, B, F, pattern):
    from cdcmdr_amd import _lib as L
    lib = L.load()
    rng = np.random.default_rng(B * 10 + F)
    idx = _pattern(pattern, B, F, rng)
    if pattern == "random_dups":
        dup = 1.0 - len(np.unique(idx[:, 0])) / B
        assert 0.25 < dup < 0.33, dup
    bufs = _buffers(B, F, cuda)
    # a scratch buffer, when given, is not needed at these sizes: the result is the same with and without one
    scratch = torch.empty(2 * F * B, dtype=torch.int64, device=cuda) if F == 3 else None
    _sort(lib, L, torch.from_numpy(idx).to(cuda), bufs, B, F, scratch)
    _check(bufs, _oracle(idx.view(np.uint32)), B)


def test_radix_sort_skips_constant_digit_passes_only(cuda):
    """Rows that differ in one byte only (each of the four in turn, the others non-zero and equal): the pass of that byte must
    run, and skipping the other three must not disturb the order."""
    from cdcmdr_amd import _lib as L
    lib = L.load()
    B, F = 2500, 4
    rng = np.random.default_rng(7)
    base = 0x5a3c1e42
    idx = np.stack([(base & ~(0xff << (8 * f))) | ((rng.integers(0, 256, size=B) >> (1 if f == 3 else 0)) << (8 * f)) for f in range(F)],
                   axis=1).astype(np.int64).astype(np.int32)
    bufs = _buffers(B, F, cuda)
    _sort(lib, L, torch.from_numpy(idx).to(cuda), bufs, B, F)
    _check(bufs, _oracle(idx.view(np.uint32)), B)


@pytest.mark.parametrize("B", SIZES)
def test_radix_sort_from_raw_ids(cuda, B):
    """cdc_embed_sort_dedupe_ids with non-zero field offsets: out-of-range ids come last as row -1, err_flag holds 1 + the
    largest offending flat position, and each call advances the step counter by exactly one and clears the accumulators."""
    from cdcmdr_amd import _lib as L
    lib = L.load()
    F = 3
    fd = np.array([1000, 1 << 20, 77], dtype=np.int64)
    lead = 5                                                # rows before the first field: every offset is non-zero
    offsets = (lead + np.concatenate([[0], np.cumsum(fd)[:-1]])).astype(np.int32)
    R = int(lead + fd.sum())
    rng = np.random.default_rng(B)
    ids = np.stack([rng.integers(0, d, size=B) for d in fd], axis=1).astype(np.int32)
    bad = [(3, 2, 10 ** 7), (B // 2, 0, -9), (B - 2, 1, R), (B - 2, 0, -(1 << 30))]      # (batch row, field, id)
    for b, f, v in bad:
        ids[b, f] = v
    rows = (ids.astype(np.int64) + offsets[None, :]).astype(np.int32)       # no wrap at these values
    rows[(rows < 0) | (rows >= R)] = -1
    assert all(rows[b, f] == -1 for b, f, _ in bad) and int((rows == -1).sum()) == len(bad)
    want = _oracle(rows.view(np.uint32))
    want_err = 1 + max(b * F + f for b, f, _ in bad)
    d_ids, d_off = torch.from_numpy(ids).to(cuda), torch.from_numpy(offsets).to(cuda)
    step = torch.tensor([41], dtype=torch.int32, device=cuda)
    acc = torch.empty(3, dtype=torch.float64, device=cuda)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for call in range(2):
        acc.fill_(3.5)
        err = torch.zeros(1, dtype=torch.int32, device=cuda)
        bufs = _buffers(B, F, cuda)
        uniq, seg, perm, cnt = bufs
        L.check(lib.cdc_embed_sort_dedupe_ids(d_ids.data_ptr(), d_off.data_ptr(), R, step.data_ptr(), acc.data_ptr(), 3, err.data_ptr(),
                                              uniq.data_ptr(), seg.data_ptr(), perm.data_ptr(), cnt.data_ptr(), None, B, F, s), "sort ids")
        _check(bufs, want, B)
        assert int(err.item()) == want_err
        assert int(step.item()) == 42 + call and float(acc.abs().sum()) == 0.0
        for f in range(F):
            n_bad = sum(1 for _, bf, _ in bad if bf == f)
            c = int(cnt[f].item())
            assert (int(uniq[f, c - 1].item()) == -1) == (n_bad > 0)
            if n_bad:
                assert int(seg[f, c - 1].item()) == B - n_bad           # the -1 rows are the last segment


def test_radix_sort_reused_workspace_and_graph_replay(cuda):
    """Three different batches in a row into the same outputs, then the launch captured in a graph and replayed twice (the
    second time on new ids in the captured input buffer): nothing carries over from one sort to the next."""
    from cdcmdr_amd import _lib as L
    lib = L.load()
    B, F = 3000, 3
    rng = np.random.default_rng(11)
    batches = [_pattern(p, B, F, rng) for p in ("high_bits", "all_equal", "random_dups", "descending", "random_dups")]
    d_idx = torch.empty((B, F), dtype=torch.int32, device=cuda)
    bufs = _buffers(B, F, cuda)
    for idx in batches[:3]:
        d_idx.copy_(torch.from_numpy(idx))
        _sort(lib, L, d_idx, bufs, B, F)
        _check(bufs, _oracle(idx.view(np.uint32)), B)
    d_idx.copy_(torch.from_numpy(batches[3]))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _sort(lib, L, d_idx, bufs, B, F)
    g.replay()
    _check(bufs, _oracle(batches[3].view(np.uint32)), B)
    d_idx.copy_(torch.from_numpy(batches[4]))
    g.replay()
    _check(bufs, _oracle(batches[4].view(np.uint32)), B)
