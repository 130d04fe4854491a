"""probe.pack_passes (pure host arithmetic) and the argument checks of cdc_eval_segments, which come before any launch."""
import ctypes as C

import pytest

from cdcmdr_amd.probe import pack_passes


def _covers_once_in_order(passes, n):
    pos = 0
    for first, last in passes:
        assert first == pos and last > first
        pos = last
    assert pos == n


def test_equal_segments_fill_passes():
    passes = pack_passes([64] * 6, 128)
    assert passes == [(0, 2), (2, 4), (4, 6)]
    _covers_once_in_order(passes, 6)


def test_cap_at_or_above_the_total_gives_one_pass():
    sizes = [3, 64, 17, 0, 5]
    assert pack_passes(sizes, sum(sizes)) == [(0, 5)]
    assert pack_passes(sizes, 10 ** 6) == [(0, 5)]


def test_a_segment_equal_to_the_cap_sits_alone():
    assert pack_passes([10, 128, 10], 128) == [(0, 1), (1, 2), (2, 3)]
    assert pack_passes([128, 128], 128) == [(0, 1), (1, 2)]


def test_zero_size_segments_stay_in_order():
    sizes = [0, 64, 0, 0, 64, 64, 0]
    passes = pack_passes(sizes, 128)
    _covers_once_in_order(passes, len(sizes))
    for first, last in passes:
        assert sum(sizes[first:last]) <= 128
    assert passes == [(0, 5), (5, 7)]
    assert pack_passes([0, 0], 128) == [(0, 2)]


def test_a_segment_larger_than_the_cap_raises():
    with pytest.raises(ValueError):
        pack_passes([64, 129, 64], 128)


def test_passes_cover_every_segment_once_in_order():
    import random
    rnd = random.Random(0)
    for _ in range(50):
        cap = rnd.randint(1, 300)
        sizes = [rnd.randint(0, cap) for _ in range(rnd.randint(1, 40))]
        passes = pack_passes(sizes, cap)
        _covers_once_in_order(passes, len(sizes))
        for k, (first, last) in enumerate(passes):
            assert sum(sizes[first:last]) <= cap
            if k + 1 < len(passes):                       # greedy: the next pass's first segment did not fit any more
                assert sum(sizes[first:last]) + sizes[last] > cap
    assert pack_passes([], 8) == []


def test_eval_segments_rejects_bad_arguments_before_any_launch():
    from cdcmdr_amd import _lib
    lib = _lib.load()
    one = C.c_void_p(16)                                  # a non-null address that is never dereferenced on the host

    def call(probs=one, ld=4, label=one, start=one, n_seg=3, loss=one, rows=10, n_cols=3):
        return lib.cdc_eval_segments(probs, ld, label, start, n_seg, None, loss, None, None, None, rows, n_cols, None)

    for kw in ({"probs": None}, {"label": None}, {"start": None}, {"loss": None}):
        assert call(**kw) == -1 and b"null pointer" in lib.cdc_last_error()
    for kw in ({"n_seg": 0}, {"n_cols": 0}, {"ld": 2}, {"rows": -1}):
        assert call(**kw) == -1 and b"bad sizes" in lib.cdc_last_error()


def test_a_cap_that_is_no_multiple_of_64_still_bounds_every_pass(monkeypatch):
    """the plan size is the cap rounded up to 64 rows, a pass still holds at most the cap (host logic: a stand-in model and metric)"""
    import torch
    from cdcmdr_amd import probe
    seen = []

    def fake_eval_segments(probs, label, sizes, cols, metric):
        seen.append((probs.shape[0], list(sizes)))
        fake_eval_segments.last_err = torch.zeros(1, dtype=torch.int32)
        return torch.zeros(len(sizes))

    class Base(torch.nn.Module):
        def forward(self, X):
            return torch.zeros(X.shape[0], 2)

    monkeypatch.setattr(probe, "eval_segments", fake_eval_segments)
    pe = probe.ProbeEval(Base(), 2, rows_cap=100)
    batches = [(torch.zeros(40, 3, dtype=torch.int32), torch.zeros(40, 1, dtype=torch.int16)) for _ in range(3)]
    pe.run(batches, [0, 1, 0], "loss")
    assert pe.B == 128 and seen == [(128, [40, 40]), (128, [40])]
    seen.clear()
    big = [(torch.zeros(120, 3, dtype=torch.int32), torch.zeros(120, 1, dtype=torch.int16))] + batches[:1]
    pe.run(big, [0, 1], "loss")                               # a single batch above the cap sits alone
    assert pe.B == 128 and seen == [(128, [120]), (128, [40])]
