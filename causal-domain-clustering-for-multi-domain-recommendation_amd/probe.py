"""Every domain's probe batch through ONE eval forward: the evaluation half of CDC's affinity-matrix update
(run.py:549-558), which the reference — and CDCTrainer without `batched_probe` — runs as one small forward and one metric call per
domain, ~150 probes x n_domain times per update.

An eval-mode forward is row-independent (BatchNorm on its running statistics, no dropout; every CDC base scores a row from that
row alone), so the domains' batches are laid end to end in one staging buffer of a FIXED size B, the base model runs once on it
(one eval plan, built once and kept), and `evaluate.eval_segments` turns the [B, n_tower] output into one figure per domain in one
launch: segment d is scored by column cols[d].  Totals beyond `rows_cap` are cut into passes of whole batches (`pack_passes`).
"""
import torch

from .evaluate import eval_segments

# Rows of one pass.  A sizing choice, not a measured optimum: about 0.8 GB of activations for PLE-3 at the reference's widths, and
# one pass for the reference's batch size 512 at 50 domains.
ROWS_CAP = 32768


def pack_passes(sizes, cap):
    """Greedy packing of consecutive segments into passes of at most `cap` rows; a segment is never split.
    -> [(first, last_exclusive), ...] covering range(len(sizes)) once, in order.  ValueError for a segment larger than cap."""
    passes, first, used = [], 0, 0
    for i, s in enumerate(sizes):
        s = int(s)
        if s < 0 or s > cap:
            raise ValueError(f"segment {i} holds {s} rows: outside [0, {cap}], the rows of one pass")
        if used + s > cap:
            passes.append((first, i))
            first, used = i, 0
        used += s
    if first < len(sizes):
        passes.append((first, len(sizes)))
    return passes


class ProbeEval:
    """base: the model whose forward(X int32 [B, F]) returns [B, n_cols_of] probabilities (CDC's base_model_instance);
    n_cols_of: the number of columns of that output (its towers); rows_cap: the most rows one pass may hold."""

    def __init__(self, base, n_cols_of, rows_cap=ROWS_CAP):
        self.base, self.n_cols, self.rows_cap = base, int(n_cols_of), int(rows_cap)
        if self.n_cols <= 0 or self.rows_cap <= 0:
            raise ValueError("n_cols_of and rows_cap must be positive")
        self.B = 0
        self._total = self._single = 0              # the largest total / single batch seen: B only ever grows
        self._X = self._y = None
        self.last_err = None                        # device int32 [1]: 1 + a bad row of a pass (see evaluate.eval_segments), never read here

    def _size(self, sizes):
        self._total = max(self._total, sum(sizes))
        self._single = max(self._single, max(sizes))
        B = max(-(-min(self.rows_cap, self._total) // 64) * 64, self._single)
        return max(B, self.B)

    def run(self, batches, cols, metric):
        """batches: [(X int32 [b_d, F], y int16 [b_d, 1] or [b_d]), ...] with ragged b_d; cols[d]: the column (tower) that scores
        batch d; metric 'loss' or 'auc'.  -> device float32 [len(batches)], nothing read back."""
        if len(cols) != len(batches) or not batches:
            raise ValueError("one column per batch, and at least one batch")
        cols = [int(c) for c in cols]
        if min(cols) < 0 or max(cols) >= self.n_cols:
            raise ValueError(f"cols must lie in [0, {self.n_cols})")
        sizes = [int(X.shape[0]) for X, _ in batches]
        X0 = batches[0][0]
        dev, F = X0.device, X0.shape[1]
        B = self._size(sizes)
        if B == 0:
            return torch.full((len(batches),), float("nan"), dtype=torch.float32, device=dev)
        if self._X is None or B != self.B or self._X.shape[1] != F or self._X.device != dev:
            self.B = B
            self._X = torch.zeros((B, F), dtype=torch.int32, device=dev)       # id 0 of every field until real rows arrive
            self._y = torch.zeros(B, dtype=torch.int16, device=dev)
        out = torch.empty(len(batches), dtype=torch.float32, device=dev)
        err = None
        was_training = self.base.training
        self.base.eval()
        try:
            with torch.no_grad():
                # B is rows_cap rounded up to 64: a pass still holds at most rows_cap rows (or one batch larger than that)
                for first, last in pack_passes(sizes, max(min(B, self.rows_cap), self._single)):
                    n = sum(sizes[first:last])
                    if n == 0:
                        out[first:last] = float("nan")
                        continue
                    torch.cat([X.to(torch.int32) for X, _ in batches[first:last]], out=self._X[:n])
                    torch.cat([y.reshape(-1).to(torch.int16) for _, y in batches[first:last]], out=self._y[:n])
                    if n < B:                                     # the tail belongs to no segment: in-range ids, nothing else
                        self._X[n:] = self._X[0]
                    probs = self.base(self._X)
                    if probs.shape != (B, self.n_cols):
                        raise ValueError(f"the model returned {tuple(probs.shape)}, not ({B}, {self.n_cols})")
                    out[first:last] = eval_segments(probs, self._y, sizes[first:last], cols[first:last], metric)
                    e = eval_segments.last_err
                    err = e if err is None else torch.maximum(err, e)
        finally:
            self.base.train(was_training)
        self.last_err = err
        return out
