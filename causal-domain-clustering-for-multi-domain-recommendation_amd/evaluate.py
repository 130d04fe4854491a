"""Evaluation path of the reference on the device: `Run.test` + `Run.evaluate_multi_domain`
(run.py:647-711).

The reference runs the model in eval mode batch by batch, moves every batch's predictions, labels and domain column to
the host (`.cpu().numpy()`, one synchronisation per batch) and calls sklearn's roc_auc_score / log_loss on the whole set
and per domain (pandas groupby).  Here the forward runs on the HIP plans (eval mode: BatchNorm on running statistics, no
dropout), predictions stay in HBM and ONE C-ABI call (`cdc_eval_metrics`) returns every figure; the only host
synchronisation is reading the result.

With a user column configured the same pass also yields GAUC — the reference's `gauc_score` (base.py:33-64): the AUC of every
user's rows, averaged over the users that have both classes, weighted by their row count or a given weight — from one more
C-ABI call (`cdc_eval_gauc`) on the same device-resident predictions.

`eval_rank` answers what stands at the top of each user's list: NDCG@K, Recall@K, Precision@K, HitRate@K and MRR@K per user, averaged
per domain and over all rows, every figure the expectation over the order of tied scores (`cdc_eval_rank`, on GAUC's sort and first
scan); `Evaluator(rank_at=(1, 10))` reports them and `Runner(select_by="mean_ndcg@10")` selects by one.
`eval_rank_ci` adds their user-clustered standard errors, the paired delta of two prediction vectors and bootstrap replicates under
`eval_bootstrap`'s user weights (`cdc_eval_rank_ci`); `Evaluator(rank_ci=True)` and `Evaluator.compare` report them.

`eval_topk` hands the ranking itself back: for every user, per domain or over all rows, the K best-scored rows, best first, no item
twice, under a total order (score, item id, row index) that does not depend on how a sort leaves ties (`cdc_eval_topk`); `TopK`
holds the lists, `TopK.merge` joins the lists of two passes, and `Evaluator.recommend` returns them for a loader.

`catalog_rows` / `catalog_topk` recommend from an item catalogue: the user x item pool is never held as a whole — a tile of it is
written (`cdc_catalog_rows`), scored by the eval forward, and folded into every context's running list of k entries
(`cdc_catalog_topk`: threshold, LDS buffer, sort under the same total order); `CatalogTopK` holds the lists, `catalog_seen` builds
the seen sets, and `Evaluator.recommend_catalog` drives the tiles.

`eval_auc_ci` adds what an AUC needs to be judged: its DeLong standard error on this evaluation set, and for two prediction
vectors over the same rows the difference of their AUCs with the standard error of that difference (`cdc_eval_auc_delong`);
`Evaluator(auc_ci=True)` and `Evaluator.compare` report them.

`eval_loss_ci` and `eval_gauc_ci` do the same for the other two headline figures: the log-loss with the standard error of its mean
(rows taken as independent) and GAUC with a user-clustered standard error (the linearised ratio estimator, clusters = users), and
for two prediction vectors over the same rows the paired difference with its standard error (`cdc_eval_loss_ci`,
`cdc_eval_gauc_ci`); `Evaluator(loss_ci=True, gauc_ci=True)` and `Evaluator.compare` report them — the log-loss delta is the one
figure that moves when a model is recalibrated.

`eval_bootstrap` covers what those analytic errors leave out: DeLong's and the log-loss's take rows as independent, the per-domain
figures share users, and so do two models on one evaluation set.  It resamples whole users — one weight per user and replicate,
applied to all of the user's rows in every domain and under both prediction vectors — and recomputes AUC, log-loss and GAUC for every
replicate on the device (`cdc_eval_bootstrap`: the rows are sorted once, the replicates reuse that order); `summarize_bootstrap`
gives the standard error and the percentile interval, `Evaluator(bootstrap=R)` reports them, mean_gauc's and the deltas of
`Evaluator.compare` included.  `eval_calibration_bootstrap` does the same for the calibration figures (pcoc, brier, ece, ece_q:
`cdc_eval_calibration_bootstrap`); `Evaluator(calibration_ci=True)` reports their intervals and the calibration deltas of `compare`.

`eval_calibration` reports whether the predicted probabilities are right, where the figures above only say how well they rank: per
domain and over all rows the ratio of predicted to observed CTR, the Brier score, and a reliability table with ECE / MCE for
equal-width and equal-mass bins (`cdc_eval_calibration`); `Evaluator(calibration=True)` and `Evaluator.calibration_table` report them.

`eval_isotonic_fit` / `eval_isotonic_apply` repair what `eval_calibration` measures: a monotone map per domain (isotonic regression of the
labels on the score, fitted on the validation split: `cdc_eval_isotonic_fit`) that is applied to the predictions of the test split
(`cdc_eval_isotonic_apply`); `Recalibration` holds a fitted map, `Evaluator.fit_recalibration` fits one and
`Evaluator(recalibration=...)` reports the recalibrated model.  `eval_platt_fit` / `eval_platt_apply` / `PlattRecalibration` are the
parametric half: sigmoid(a z + b) of the logit-scale score per domain — Platt scaling, temperature scaling (a alone) and the bias
shift (b alone) that undoes negative down-sampling — fitted by Newton steps on the device (`cdc_eval_platt_fit`), for domains too
small for an isotonic map.

`eval_segments` serves CDC's matrix update (run.py:549-558) instead: the metric of every contiguous row segment of ONE forward's
raw output, each segment scored by its own tower column (`cdc_eval_segments`; probe.py lays the domains' batches out that way).
"""
import collections
import ctypes as C
import math

import torch

from . import _lib as L


def _need_device(name, t):
    if not t.is_cuda:
        raise L.HipExtensionError(f"{name} needs device tensors; there is no CPU fallback")


def _flat(t, dtype, dev=None):
    """t as a contiguous 1-D tensor of dtype (on dev); a tensor that already is one passes through without a torch call"""
    if t.dtype is dtype and t.dim() == 1 and t.is_contiguous() and (dev is None or t.device == dev):
        return t
    return t.reshape(-1).to(device=dev, dtype=dtype).contiguous()


def _rows(name, pred, label=None, pred_b=None, max_rows=None):
    """The row vectors of a call: device refusal, flattening, length checks -> (pred f32, label int16 or None, pred_b f32 or None, n).
    max_rows: (limit, what the limit protects), checked between the labels and pred_b."""
    _need_device(name, pred)
    pred = _flat(pred, torch.float32)
    n = pred.numel()
    if label is not None:
        label = _flat(label, torch.int16)
        if label.numel() != n:
            raise ValueError(f"{n} predictions but {label.numel()} labels")
    if max_rows is not None and n > max_rows[0]:
        raise ValueError(f"{n} rows exceed the {max_rows[0]} {max_rows[1]}")
    if pred_b is not None:
        pred_b = _flat(pred_b, torch.float32, pred.device)
        if pred_b.numel() != n:
            raise ValueError(f"{n} predictions but {pred_b.numel()} in pred_b")
    return pred, label, pred_b, n


def _id_column(col, n, what):
    """int32 [n] or a strided column view (X[:, idx]) -> (tensor, element stride)"""
    if col.dtype != torch.int32:
        col = col.to(torch.int32)
    col = col.reshape(-1) if col.dim() > 1 and col.is_contiguous() else col
    if col.dim() != 1 or col.numel() != n:
        raise ValueError(f"{what} must hold one entry per prediction")
    return col, col.stride(0)


def _id_arg(col, n, what):
    """an optional id column -> (tensor or None, element stride, address or None)"""
    if col is None:
        return None, 0, None
    col, ld = _id_column(col, n, what)
    return col, ld, col.data_ptr()


def _domain_arg(domain, n, n_domain):
    if domain is None and n_domain != 1:
        raise ValueError("n_domain > 1 needs the domain column")
    return _id_arg(domain, n, "domain")


def _user_weight_arg(w, n_user, dev, what="users"):
    """-> (f64 [n_user] on the device or None, address or None)"""
    if w is None:
        return None, None
    w = torch.as_tensor(w, dtype=torch.float64).to(dev).reshape(-1).contiguous()
    if w.numel() != n_user:
        raise ValueError(f"user_weight holds {w.numel()} entries for {n_user} {what}")
    return w, w.data_ptr()


def _group_ids_ok(n_user, n_domain, n_seg, n_seg_text):
    """n_seg * n_user (domain, user) groups must fit the upper half of a sort key; n_seg_text: how the message spells n_seg"""
    if n_user <= 0 or n_domain <= 0:
        raise ValueError(f"n_user={n_user} and n_domain={n_domain} must be positive")
    if n_seg * n_user > 1 << 32:
        raise ValueError(f"{n_seg_text} * n_user = {n_seg * n_user} group ids exceed 2^32, the upper half of a sort key")


def _ptr(t):
    return None if t is None else t.data_ptr()


def _call(owner, entry, args, dev, size=None, refused=None, tail=()):
    """One C-ABI launch on the current stream: entry(*args, error word, *tail[, workspace, bytes]).  size: the name of the entry's
    workspace query and its arguments (None: the entry takes no workspace); `refused` is the RuntimeError's text when the query
    answers <= 0.  The error word is kept as owner.last_err."""
    lib = L.load()
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    args = args + (err.data_ptr(),) + tail
    if size is not None:
        nbytes = getattr(lib, size[0])(*size[1:])
        if nbytes <= 0:
            raise RuntimeError(refused or f"{size[0]} failed")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        args += (ws.data_ptr(), nbytes)
    L.launch(entry, getattr(lib, entry), args, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    owner.last_err = err


def eval_metrics(pred, label, domain=None, n_domain=1):
    """pred f32 [n], label int16 [n] (0/1), domain int32 [n] or a strided column view (e.g. X[:, domain_idx]).
    Returns (auc, loss, rows, positives): device tensors with n_domain + 1 entries each — domains 0..n_domain-1, then ALL
    rows.  NaN where a segment is empty or holds a single class.  No host synchronisation."""
    pred, label, _, n = _rows("eval_metrics", pred, label)
    domain, ld, domain_p = _domain_arg(domain, n, n_domain)
    dev = pred.device
    seg = n_domain + 1
    out = torch.empty(2 * seg, dtype=torch.float64, device=dev)
    counts = torch.empty(2 * seg, dtype=torch.int64, device=dev)
    _call(eval_metrics, "cdc_eval_metrics", (pred.data_ptr(), label.data_ptr(), domain_p, ld, n, n_domain, out.data_ptr(), counts.data_ptr()),
          dev, ("cdc_eval_workspace_bytes", n, n_domain))
    return out[:seg], out[seg:], counts[:seg], counts[seg:]


def eval_segments(probs, label, seg_sizes, seg_col=None, metric="loss"):
    """Per-segment metric of CDC's probe evaluation: probs f32 [rows, n_cols] (a model's raw output, every tower's probability; a
    row-strided view is read in place), label int16 [rows] (0/1); seg_sizes: host sequence of row counts of consecutive row
    segments (rows past their sum are padding and never looked at); seg_col: host sequence, the column segment s is scored by
    (None = column 0).  metric "loss": the mean BCE of every segment (F.binary_cross_entropy's arithmetic), NaN for an empty one —
    ONE launch (`cdc_eval_segments`); "auc": the same launch hands every row's selected probability and segment to
    `cdc_eval_metrics`, NaN for an empty or single-class segment.  Returns a device float32 [n_seg] tensor; nothing is read back:
    the error word (1 + a row inside a segment with a NaN probability or a label outside {0, 1}) is kept as
    `eval_segments.last_err`."""
    if metric not in ("loss", "auc"):
        raise ValueError(f"metric must be 'loss' or 'auc', not {metric!r}")
    _need_device("eval_segments", probs)
    if probs.dim() == 1:
        probs = probs.reshape(-1, 1)
    if probs.dim() != 2:
        raise ValueError("probs must be [rows, n_cols]")
    rows, n_cols = probs.shape
    if probs.dtype != torch.float32 or (n_cols > 1 and probs.stride(1) != 1) or (rows > 1 and probs.stride(0) < n_cols):
        probs = probs.to(torch.float32).contiguous()
    ld = max(probs.stride(0), n_cols)
    label = label.reshape(-1).to(torch.int16).contiguous()
    if label.numel() != rows:
        raise ValueError(f"{rows} rows of probabilities but {label.numel()} labels")
    sizes = [int(s) for s in seg_sizes]
    n_seg = len(sizes)
    if n_seg == 0 or min(sizes) < 0:
        raise ValueError("seg_sizes must hold at least one segment and no negative size")
    starts = [0]
    for s in sizes:
        starts.append(starts[-1] + s)
    n = starts[-1]
    if n > rows:
        raise ValueError(f"the segments hold {n} rows, probs only {rows}")
    cols = [0] * n_seg if seg_col is None else [int(c) for c in seg_col]
    if len(cols) != n_seg or min(cols) < 0 or max(cols) >= n_cols:
        raise ValueError(f"seg_col must hold one column in [0, {n_cols}) per segment")
    dev = probs.device
    # bounds and columns travel in one copy from pinned memory: stream-ordered, the host does not wait for the device
    meta = torch.tensor(starts + cols, dtype=torch.int32, pin_memory=True).to(dev, non_blocking=True)
    loss = torch.empty(n_seg, dtype=torch.float64, device=dev)
    want_auc = metric == "auc" and n > 0
    sel = torch.empty(n, dtype=torch.float32, device=dev) if want_auc else None
    seg = torch.empty(n, dtype=torch.int32, device=dev) if want_auc else None
    _call(eval_segments, "cdc_eval_segments", (probs.data_ptr(), ld, label.data_ptr(), meta.data_ptr(), n_seg, meta[n_seg + 1:].data_ptr(),
                                               loss.data_ptr(), _ptr(sel), _ptr(seg)), dev, tail=(rows, n_cols))
    if metric == "loss":
        return loss.to(torch.float32)
    if not want_auc:
        return torch.full((n_seg,), math.nan, dtype=torch.float32, device=dev)
    return eval_metrics(sel, label[:n], seg, n_seg)[0][:n_seg].to(torch.float32)


def eval_gauc(pred, label, user, n_user, domain=None, n_domain=1, user_weight=None):
    """GAUC (base.py:33-64, gauc_score) per domain and over all rows.  pred f32 [n], label int16 [n] (0/1); user and domain int32
    [n] or strided column views (X[:, user_idx], X[:, domain_idx]) with ids in [0, n_user) / [0, n_domain); user_weight: f64
    [n_user] (positive), or None for gauc_score's default, the user's row count.
    Returns (gauc f64, counted i64, left_out i64): device tensors with n_domain + 1 entries each — domains 0..n_domain-1 (their rows
    grouped by user), then ALL rows grouped by user across domains; counted / left_out are the users with both classes / with a
    single class.  NaN where no user is counted (the reference divides by zero there).  No host synchronisation."""
    n_user, n_domain = int(n_user), int(n_domain)
    _group_ids_ok(n_user, n_domain, n_domain + 1, "(n_domain + 1)")
    pred, label, _, n = _rows("eval_gauc", pred, label)
    user, ld_user = _id_column(user, n, "user")
    domain, ld_domain, domain_p = _domain_arg(domain, n, n_domain)
    dev = pred.device
    user_weight, weight_p = _user_weight_arg(user_weight, n_user, dev)
    seg = n_domain + 1
    out = torch.empty(seg, dtype=torch.float64, device=dev)
    counts = torch.empty(2 * seg, dtype=torch.int64, device=dev)
    _call(eval_gauc, "cdc_eval_gauc", (pred.data_ptr(), label.data_ptr(), user.data_ptr(), ld_user, n_user, domain_p, ld_domain, n_domain,
                                       weight_p, n, out.data_ptr(), counts.data_ptr()), dev, ("cdc_eval_gauc_workspace_bytes", n, n_domain, n_user))
    return out, counts[:seg], counts[seg:]


Rank = collections.namedtuple("Rank", "ndcg recall precision hit mrr counted left_out")
RANK_FIGURES = ("ndcg", "recall", "precision", "hit", "mrr")
RANK_MAX_K, RANK_MAX_NK = 1024, 8
_rank_tables = {}


def _rank_ks(ks):
    """an int or a sequence of ints -> the tuple of cut-offs, checked against cdc_eval_rank's limits"""
    ks = (ks,) if isinstance(ks, int) and not isinstance(ks, bool) else tuple(ks)
    if not 1 <= len(ks) <= RANK_MAX_NK:
        raise ValueError(f"ks={ks!r} holds {len(ks)} cut-offs: 1 to {RANK_MAX_NK} are served")
    for k in ks:
        if isinstance(k, bool) or int(k) != k or not 1 <= k <= RANK_MAX_K:
            raise ValueError(f"ks={ks!r}: the cut-off {k!r} is no integer in [1, {RANK_MAX_K}]")
    ks = tuple(int(k) for k in ks)
    for a, b in zip(ks, ks[1:]):
        if b <= a:
            raise ValueError(f"ks={ks!r} must be strictly increasing: {b} follows {a}")
    return ks


def _rank_ks_dev(ks, dev):
    """the cut-offs as an int32 device tensor, cached per (device, ks); from pinned memory, as rank_discounts' table"""
    key = ("ks", str(dev), ks)
    if key not in _rank_tables:
        _rank_tables[key] = torch.tensor(ks, dtype=torch.int32, pin_memory=True).to(dev, non_blocking=True)
    return _rank_tables[key]


def rank_discounts(k_max, device=None):
    """The cumulative discounts of NDCG, f64 [k_max + 1]: D[0] = 0, D[r + 1] = D[r] + 1 / log2(r + 2), added sequentially in float64 on
    the host — D[min(P, K)] is the ideal DCG of P positives.  Cached per (device, k_max); device None: a host tensor."""
    k_max = int(k_max)
    if not 1 <= k_max <= RANK_MAX_K:
        raise ValueError(f"k_max={k_max} must lie in [1, {RANK_MAX_K}]")
    key = ("D", None if device is None else str(device), k_max)
    if key not in _rank_tables:
        table = [0.0]
        for r in range(k_max):
            table.append(table[-1] + 1.0 / math.log2(r + 2))
        if device is None:
            _rank_tables[key] = torch.tensor(table, dtype=torch.float64)
        else:                                                  # from pinned memory: stream-ordered, the host does not wait for the device
            _rank_tables[key] = torch.tensor(table, dtype=torch.float64, pin_memory=True).to(device, non_blocking=True)
    return _rank_tables[key]


def eval_rank(pred, label, user, n_user, domain=None, n_domain=1, ks=(10,), user_weight=None):
    """Per-user top-K ranking figures per domain and over all rows: NDCG@K, Recall@K, Precision@K, HitRate@K and MRR@K for every K of
    `ks` (1 to 8 strictly increasing integers in [1, 1024]).  Inputs and groups as `eval_gauc`: a group is a user's rows of a domain,
    or all of a user's rows for the last entry.  A group is ranked by descending score and every figure is the expectation over a
    uniformly random order of the rows that tie in score (-0.0 ties with +0.0), so no figure depends on how a sort left tied rows;
    the definitions are in include/cdcmdr.h (`cdc_eval_rank`).  A segment's value is sum_g w_g m_g / sum_g w_g over its groups with at
    least one positive; w_g = user_weight[user], or 1 when user_weight is None: the MACRO average over users, as these figures are
    reported in the literature — unlike `eval_gauc`, whose default weight is the user's row count.
    Returns Rank(ndcg, recall, precision, hit, mrr, counted, left_out): the figures f64 device tensors [len(ks), n_domain + 1], NaN
    where no group is counted; counted / left_out i64 [n_domain + 1], the groups with / without a positive.  The same rows in any
    order give the same bits.  No host synchronisation; the error word (as `eval_gauc`'s) is kept as `eval_rank.last_err`."""
    n_user, n_domain = int(n_user), int(n_domain)
    _group_ids_ok(n_user, n_domain, n_domain + 1, "(n_domain + 1)")
    ks = _rank_ks(ks)
    pred, label, _, n = _rows("eval_rank", pred, label)
    user, ld_user = _id_column(user, n, "user")
    domain, ld_domain, domain_p = _domain_arg(domain, n, n_domain)
    dev = pred.device
    user_weight, weight_p = _user_weight_arg(user_weight, n_user, dev)
    ks_dev, disc = _rank_ks_dev(ks, dev), rank_discounts(ks[-1], dev)
    seg, n_k = n_domain + 1, len(ks)
    out = torch.empty((len(RANK_FIGURES), n_k, seg), dtype=torch.float64, device=dev)
    counts = torch.empty((2, seg), dtype=torch.int64, device=dev)
    _call(eval_rank, "cdc_eval_rank", (pred.data_ptr(), label.data_ptr(), user.data_ptr(), ld_user, n_user, domain_p, ld_domain, n_domain,
                                       weight_p, ks_dev.data_ptr(), n_k, disc.data_ptr(), n, out.data_ptr(), counts.data_ptr()), dev,
          ("cdc_eval_rank_workspace_bytes", n, n_domain, n_user, n_k),
          f"cdc_eval_rank_workspace_bytes refused n={n}, n_domain={n_domain}, n_user={n_user}, n_k={n_k}")
    return Rank(out[0], out[1], out[2], out[3], out[4], counts[0], counts[1])


TOPK_MAX_K = (1 << 31) - 1


class TopK:
    """The per-user top-K lists of `eval_topk` (the definitions are in include/cdcmdr.h, `cdc_eval_topk`).  G groups with at least one
    surviving row, in ascending (domain, user) order, and E entries in all lists together:
      domain, user  int32 [G]: the group's ids (domain is 0 throughout when the lists are over all rows by user)
      start         int32 [G + 1]: group j's entries are start[j]:start[j + 1]; start[G] == E
      rows          int32 [G]: the group's survivors BEFORE the cut — larger than the list's length where the list was truncated
      row, score    int32 / f32 [E]: the input row index and its score (bit-copied), best first inside a group
      item, label   [E] or None: the entries' item ids (when the call de-duplicated by item) and labels (`Evaluator.recommend`)
      n_out         int64 [2] device tensor (G, E);  k: the cut;  n, n_user, n_domain: the call's sizes;  err: the device error word
    synced: the counts were read and every tensor is sliced to G or E.  Otherwise (`eval_topk(sync=False)`) nothing was read back: the
    tensors keep their capacity n (start: n + 1), what stands past n_out's counts is unspecified, and `dense`, `lists` and `merge`
    are not served."""

    def __init__(self, domain, user, start, rows, row, score, n_out, k, n, n_user, n_domain, item=None, label=None, err=None, synced=True):
        self.domain, self.user, self.start, self.rows, self.row, self.score = domain, user, start, rows, row, score
        self.n_out, self.k, self.n, self.n_user, self.n_domain = n_out, int(k), int(n), int(n_user), int(n_domain)
        self.item, self.label, self.err, self.synced = item, label, err, bool(synced)

    def _need_sync(self, what):
        if not self.synced:
            raise ValueError(f"TopK.{what} needs the counts: call eval_topk with sync=True")

    def _group_of_entry(self):
        """int64 [E]: the group index of every entry"""
        start = self.start.to(torch.int64)
        return torch.repeat_interleave(torch.arange(self.domain.numel(), device=start.device), start[1:] - start[:-1],
                                       output_size=self.row.numel())

    def dense(self, fill=-1):
        """-> (row int32 [G, k], score f32 [G, k]): list j in line j, padded with `fill` and NaN.  k is the call's cut: ask for the
        lists with the k the table should have."""
        self._need_sync("dense")
        G, dev = self.domain.numel(), self.row.device
        row = torch.full((G, self.k), fill, dtype=torch.int32, device=dev)
        score = torch.full((G, self.k), math.nan, dtype=torch.float32, device=dev)
        if self.row.numel():
            grp = self._group_of_entry()
            pos = torch.arange(self.row.numel(), device=dev) - self.start.to(torch.int64)[grp]
            row[grp, pos] = self.row
            score[grp, pos] = self.score
        return row, score

    def lists(self):
        """-> host dict {(domain, user): (rows, scores)}, two lists per group, for inspection"""
        self._need_sync("lists")
        dom, usr, start = self.domain.cpu().tolist(), self.user.cpu().tolist(), self.start.cpu().tolist()
        row, score = self.row.cpu().tolist(), self.score.cpu().tolist()
        return {(dom[j], usr[j]): (row[start[j]:start[j + 1]], score[start[j]:start[j + 1]]) for j in range(len(dom))}

    @staticmethod
    def merge(a, b, k=None, row_offset=None):
        """The lists of two passes over disjoint row sets as one: both entry sets concatenated (a's first), b's row indices shifted by
        `row_offset` (default a.n: b's rows follow a's), and ranked again under the same rules by one more `eval_topk` call over the
        E_a + E_b entries.  k: the cut of the result (default min(a.k, b.k)).  For k <= min(a.k, b.k) the result's domain, user, start,
        row, score, item and label equal those of `eval_topk` over the concatenated inputs: a row outside its pass's first k cannot
        stand inside the first k of the union, de-duplication included (a better row of the same item is in the same list or has
        displaced it), and an entry's place in the concatenation orders like its row index wherever the two can tie.  `rows` counts
        the survivors among the MERGED ENTRIES — the rows a pass has cut are gone — so it equals the one-call value only for groups
        no pass truncated.  Both need the same n_user, n_domain and either both or neither the item ids."""
        a._need_sync("merge")
        b._need_sync("merge")
        if (a.n_user, a.n_domain) != (b.n_user, b.n_domain):
            raise ValueError(f"merge: the lists are over (n_domain, n_user) = {(a.n_domain, a.n_user)} and {(b.n_domain, b.n_user)}")
        if (a.item is None) != (b.item is None):
            raise ValueError("merge: one side carries item ids and the other does not")
        k = min(a.k, b.k) if k is None else int(k)
        off = a.n if row_offset is None else int(row_offset)
        if off < a.n or off + b.n >= 1 << 31:                   # b's rows behind a's: ties then break as over the concatenated rows
            raise ValueError(f"merge: row_offset={off} must put b's {b.n} rows behind a's {a.n} and below 2^31")
        n = off + b.n
        ga, gb = a._group_of_entry(), b._group_of_entry()
        orig = torch.cat([a.row, b.row + off])
        if orig.numel() == 0:
            return TopK(a.domain, a.user, a.start, a.rows, a.row, a.score, a.n_out, k, n, a.n_user, a.n_domain, a.item, a.label, a.err)
        item = None if a.item is None else torch.cat([a.item, b.item])
        m = eval_topk(torch.cat([a.score, b.score]), torch.cat([a.user[ga], b.user[gb]]), a.n_user,
                      torch.cat([a.domain[ga], b.domain[gb]]), a.n_domain, item, k)
        pos = m.row.to(torch.int64)
        m.row, m.n = orig[pos], n
        if a.label is not None and b.label is not None:
            m.label = torch.cat([a.label, b.label])[pos]
        return m


def eval_topk(pred, user, n_user, domain=None, n_domain=1, item=None, k=10, sync=True):
    """Per-user top-K recommendation lists: for every (domain, user) group — every user when `domain` is None — the k best-scored rows,
    best first, no item twice.  pred f32 [n]; user, domain and item int32 [n] or strided column views (X[:, idx]) with user in
    [0, n_user), domain in [0, n_domain) and item >= 0.  Inside a group: descending score (-0.0 ties with +0.0), equal scores by
    ascending item id (when `item` is given), then by ascending row index; with `item`, of a group's rows with one item only the first
    in that order survives; the first min(k, survivors) rows are the list (`cdc_eval_topk`; k in [1, 2^31 - 1], a k above every
    group's size returns full rankings).  A row with a NaN score or an id out of range is in no list, and the error word (1 + the
    largest such row index) is kept as `eval_topk.last_err` and as the result's `err`.
    Returns a `TopK`.  sync=True reads the two counts once and slices every tensor to them; sync=False reads nothing back (the tensors
    keep capacity n and `n_out` stays on the device): the call can be captured in a graph.  The same input gives the same bits."""
    n_user, n_domain = int(n_user), int(n_domain)
    _group_ids_ok(n_user, n_domain, n_domain, "n_domain")
    if isinstance(k, bool) or int(k) != k or not 1 <= k <= TOPK_MAX_K:
        raise ValueError(f"k={k!r} is no integer in [1, {TOPK_MAX_K}]")
    k = int(k)
    pred, _, _, n = _rows("eval_topk", pred)
    user, ld_user = _id_column(user, n, "user")
    domain, ld_domain, domain_p = _domain_arg(domain, n, n_domain)
    item, ld_item, item_p = _id_arg(item, n, "item")
    dev = pred.device
    n_out = torch.empty(2, dtype=torch.int64, device=dev)
    groups = torch.empty((3, n), dtype=torch.int32, device=dev)               # domain, user, rows
    start = torch.empty(n + 1, dtype=torch.int32, device=dev)
    row = torch.empty(n, dtype=torch.int32, device=dev)
    score = torch.empty(n, dtype=torch.float32, device=dev)
    _call(eval_topk, "cdc_eval_topk", (pred.data_ptr(), user.data_ptr(), ld_user, n_user, domain_p, ld_domain, n_domain, item_p, ld_item, k, n,
                                       n_out.data_ptr(), groups[0].data_ptr(), groups[1].data_ptr(), start.data_ptr(), groups[2].data_ptr(),
                                       row.data_ptr(), score.data_ptr()), dev, ("cdc_eval_topk_workspace_bytes", n, n_domain, n_user, int(item is not None)),
          f"cdc_eval_topk_workspace_bytes refused n={n}, n_domain={n_domain}, n_user={n_user}")
    err = eval_topk.last_err
    if not sync:
        # entries past E are unspecified: the gather stays inside the column whatever stands there
        it = None if item is None else item[row.clamp(0, n - 1).to(torch.int64)]
        return TopK(groups[0], groups[1], start, groups[2], row, score, n_out, k, n, n_user, n_domain, it, None, err, synced=False)
    G, E = n_out.cpu().tolist()                                              # the one read
    row = row[:E]
    it = None if item is None else item[row.to(torch.int64)]
    return TopK(groups[0, :G], groups[1, :G], start[:G + 1], groups[2, :G], row, score[:E], n_out, k, n, n_user, n_domain, it, None, err)


CATALOG_MAX_K = L.CATALOG_MAX_K


def _catalog_k(k):
    if isinstance(k, bool) or int(k) != k or not 1 <= k <= CATALOG_MAX_K:
        raise ValueError(f"k={k!r} is no integer in [1, {CATALOG_MAX_K}]")
    return int(k)


def _id_matrix(t, what):
    """int32 [rows, cols] whose columns are contiguous -> (tensor, row stride); a column vector may come as 1-D"""
    if t.dim() == 1:
        t = t.reshape(-1, 1)
    if t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError(f"{what} must be a non-empty 2-D id matrix, not {tuple(t.shape)}")
    if t.dtype != torch.int32:
        t = t.to(torch.int32)
    if t.stride(1) != 1 or t.stride(0) < t.shape[1]:
        t = t.contiguous()
    return t, t.stride(0)


class CatalogTopK:
    """Every context's running list of the k best catalogue items (the definitions are in include/cdcmdr.h, `cdc_catalog_topk`):
      item, cat  int32 [U, k]: the entries' item ids and catalogue row indices, best first; -1 past the list's end
      score      f32 [U, k]: their scores, bit-copied; NaN past the end
      n          int32 [U]: the lists' lengths, min(k, survivors)
      k          the cut;  err: the device error word of the calls that filled it (1 + the largest context with a NaN score or a
                 negative item id among its candidates), zeroed by `empty`
    `catalog_topk` folds a tile of scores into it in place."""

    def __init__(self, item, cat, score, n, k, err=None):
        self.item, self.cat, self.score, self.n, self.k, self.err = item, cat, score, n, int(k), err

    @classmethod
    def empty(cls, U, k, device):
        k, U = _catalog_k(k), int(U)
        if not 1 <= U < 1 << 31:
            raise ValueError(f"U={U} contexts lie outside [1, 2^31)")
        return cls(torch.full((U, k), -1, dtype=torch.int32, device=device), torch.full((U, k), -1, dtype=torch.int32, device=device),
                   torch.full((U, k), math.nan, dtype=torch.float32, device=device), torch.zeros(U, dtype=torch.int32, device=device), k,
                   torch.zeros(1, dtype=torch.int32, device=device))

    def lists(self):
        """-> host dict {u: (items, scores)}, two lists per context, for inspection"""
        n, item, score = self.n.cpu().tolist(), self.item.cpu().tolist(), self.score.cpu().tolist()
        return {u: (item[u][:n[u]], score[u][:n[u]]) for u in range(len(n))}


def catalog_seen(context_index, item, U):
    """(context, item) pairs, in any order and with repeats, -> (seen_start int32 [U + 1], seen_item int32 [S]): the CSR form
    `catalog_topk` takes, every context's slice ascending.  One torch sort; works on host or device tensors and stays on theirs."""
    U = int(U)
    ctx = torch.as_tensor(context_index).reshape(-1).to(torch.int64)
    it = torch.as_tensor(item).reshape(-1).to(device=ctx.device, dtype=torch.int64)
    if ctx.numel() != it.numel():
        raise ValueError(f"{ctx.numel()} context indices but {it.numel()} items")
    if ctx.numel() >= 1 << 31:
        raise ValueError(f"{ctx.numel()} seen pairs reach 2^31")
    if ctx.numel() and (int(ctx.min()) < 0 or int(ctx.max()) >= U):
        raise ValueError(f"a context index lies outside [0, {U})")
    key = torch.sort((ctx << 32) | (it + (1 << 31)))[0]                     # the item biased into [0, 2^32): ascending like the int32
    start = torch.zeros(U + 1, dtype=torch.int64, device=ctx.device)
    start[1:] = torch.cumsum(torch.bincount(ctx, minlength=U), 0)
    return start.to(torch.int32), ((key & 0xffffffff) - (1 << 31)).to(torch.int32)


def catalog_rows(context, catalog, item_cols, u0, ub, i0, ib, group_of_domain=None, domain_col=None, err=None):
    """The tile [u0, u0 + ub) x [i0, i0 + ib) of the user x item pool (`cdc_catalog_rows`): row (u - u0) * ib + (i - i0) is context u
    (int32 [U, F], rows may be strided) with X[item_cols[c]] = catalog[i, c] (int32 [I, C]).  -> (X int32 [ub * ib, F], group, domain):
    domain, with domain_col, is X's domain column as a contiguous int32 vector; group, with group_of_domain (int64 [n_domain]) as well,
    is int64 [ub * ib] = group_of_domain[domain] — a domain outside the table gives group 0 and sets the error word (1 + the largest
    such context; `err`, an int32 [1] device tensor to share between calls, or a fresh one; kept as `catalog_rows.last_err`).
    Nothing is read back."""
    lib = L.load()
    _need_device("catalog_rows", context)
    context, ld_context = _id_matrix(context, "context")
    catalog, ld_catalog = _id_matrix(catalog, "catalog")
    (U, F), (I, n_cols) = context.shape, catalog.shape
    cols = [int(c) for c in item_cols]
    if len(cols) != n_cols:
        raise ValueError(f"{len(cols)} item_cols for a catalogue of {n_cols} columns")
    if len(set(cols)) != n_cols or min(cols) < 0 or max(cols) >= F:
        raise ValueError(f"item_cols={cols} must be distinct columns in [0, {F})")
    if group_of_domain is not None and domain_col is None:
        raise ValueError("the group output needs domain_col, the column that holds a row's domain")
    dev, rows = context.device, int(ub) * int(ib)
    if not (0 <= u0 and 1 <= ub and u0 + ub <= U and 0 <= i0 and 1 <= ib and i0 + ib <= I and rows < 1 << 31):
        raise ValueError(f"tile [{u0}, {u0 + ub}) x [{i0}, {i0 + ib}) lies outside [0, {U}) x [0, {I}) or holds 2^31 rows")
    X = torch.empty((rows, F), dtype=torch.int32, device=dev)
    group = domain = None
    n_domain = 0
    if group_of_domain is not None:
        group_of_domain = _flat(torch.as_tensor(group_of_domain), torch.int64, dev)
        n_domain = group_of_domain.numel()
        group = torch.empty(rows, dtype=torch.int64, device=dev)
    if domain_col is not None:
        domain = torch.empty(rows, dtype=torch.int32, device=dev)
    if err is None:
        err = torch.zeros(1, dtype=torch.int32, device=dev)
    L.launch("cdc_catalog_rows", lib.cdc_catalog_rows,
             (context.data_ptr(), ld_context, U, catalog.data_ptr(), ld_catalog, I, (C.c_int32 * len(cols))(*cols), len(cols), F, int(u0),
              int(ub), int(i0), int(ib), X.data_ptr(), _ptr(group), _ptr(group_of_domain), n_domain, -1 if domain_col is None else int(domain_col),
              _ptr(domain), err.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    catalog_rows.last_err = err
    return X, group, domain


def catalog_topk(state, score, catalog, u0, ub, i0, ib, seen=None):
    """Folds the scores of the tile [u0, u0 + ub) x [i0, i0 + ib) — score f32 [ub * ib], context-major, the model's output for
    `catalog_rows`' tile — into the running lists `state` (a `CatalogTopK`), in place (`cdc_catalog_topk`): every context of the tile
    keeps the first k, by descending score (-0.0 ties with +0.0), then item id, then catalogue row, of its list so far and the tile's
    candidates.  catalog: the int32 [I, C] catalogue (column 0 is the item id) or the id column alone.  seen: None or
    (seen_start int32 [U + 1], seen_item int32 [S]) as `catalog_seen` returns them: a candidate whose id is in its context's slice is
    left out silently.  A NaN score or a negative id is left out and sets `state.err` (1 + the largest such context; also kept as
    `catalog_topk.last_err`).  Folding disjoint item tiles in any order gives the bits of one call over all items.  Nothing is read
    back; returns `state`."""
    lib = L.load()
    _need_device("catalog_topk", score)
    dev = score.device
    score = _flat(score, torch.float32, dev)
    catalog, ld_catalog = _id_matrix(catalog, "catalog")
    U, I = state.n.numel(), catalog.shape[0]
    if score.numel() != int(ub) * int(ib):
        raise ValueError(f"{score.numel()} scores for a tile of {ub} x {ib}")
    if not (0 <= u0 and 1 <= ub and u0 + ub <= U and 0 <= i0 and 1 <= ib and i0 + ib <= I):
        raise ValueError(f"tile [{u0}, {u0 + ub}) x [{i0}, {i0 + ib}) lies outside [0, {U}) x [0, {I})")
    seen_start = seen_item = None
    n_seen = 0
    if seen is not None and seen[1].numel():
        seen_start, seen_item = _flat(seen[0], torch.int32, dev), _flat(seen[1], torch.int32, dev)
        if seen_start.numel() != U + 1:
            raise ValueError(f"seen_start holds {seen_start.numel()} entries for {U} contexts")
        n_seen = seen_item.numel()
    if state.err is None:
        state.err = torch.zeros(1, dtype=torch.int32, device=dev)
    L.launch("cdc_catalog_topk", lib.cdc_catalog_topk,
             (score.data_ptr(), catalog.data_ptr(), ld_catalog, U, I, int(u0), int(ub), int(i0), int(ib), _ptr(seen_start), _ptr(seen_item),
              n_seen, state.k, state.item.data_ptr(), state.cat.data_ptr(), state.score.data_ptr(), state.n.data_ptr(), state.err.data_ptr()),
             C.c_void_p(torch.cuda.current_stream().cuda_stream))
    catalog_topk.last_err = state.err
    return state


def _segment_ci(owner, name, entry, pred, label, domain, n_domain, pred_b):
    """eval_auc_ci and eval_loss_ci: the same arguments and outputs -> (out [2 or 6, seg], counts [2 seg], seg, paired)"""
    pred, label, pred_b, n = _rows(name, pred, label, pred_b)
    n_domain = int(n_domain)
    domain, ld, domain_p = _domain_arg(domain, n, n_domain)
    dev = pred.device
    seg = n_domain + 1
    paired = pred_b is not None
    out = torch.empty((6 if paired else 2) * seg, dtype=torch.float64, device=dev)
    counts = torch.empty(2 * seg, dtype=torch.int64, device=dev)
    _call(owner, entry, (pred.data_ptr(), _ptr(pred_b), label.data_ptr(), domain_p, ld, n, n_domain, out.data_ptr(), counts.data_ptr()), dev,
          (f"{entry}_workspace_bytes", n, n_domain, int(paired)), f"{entry}_workspace_bytes refused n={n}, n_domain={n_domain}")
    return out.reshape(-1, seg), counts, seg, paired


AucCI = collections.namedtuple("AucCI", "auc var rows positives")
AucCIPaired = collections.namedtuple("AucCIPaired", "auc var rows positives auc_b var_b delta var_delta")


def eval_auc_ci(pred, label, domain=None, n_domain=1, pred_b=None):
    """AUC with its DeLong variance (DeLong, DeLong & Clarke-Pearson 1988) per domain and over all rows; inputs as `eval_metrics`
    (domain: int32 [n] or a strided column view).  Returns a namedtuple of device tensors with n_domain + 1 entries each —
    domains 0..n_domain-1, then ALL rows: `auc`, `var` (f64), `rows`, `positives` (i64); `auc` is `eval_metrics`' figure bit for
    bit.  With `pred_b` (a second prediction vector over the same rows) also `auc_b`, `var_b`, `delta` = auc - auc_b and
    `var_delta`, the variance of the PAIRED difference (formed from the rows' placement differences: far below var + var_b when
    the two vectors are close).  A standard error is `var.sqrt()`.  `auc` / `delta` are NaN for an empty or single-class segment,
    a variance is NaN when a class has fewer than two rows.  No host synchronisation; the error word (1 + a row with a NaN
    prediction in either vector, a label outside {0, 1} or a domain outside range) is kept as `eval_auc_ci.last_err`."""
    o, counts, seg, paired = _segment_ci(eval_auc_ci, "eval_auc_ci", "cdc_eval_auc_delong", pred, label, domain, n_domain, pred_b)
    if paired:
        return AucCIPaired(o[0], o[1], counts[:seg], counts[seg:], o[2], o[3], o[4], o[5])
    return AucCI(o[0], o[1], counts[:seg], counts[seg:])


LossCI = collections.namedtuple("LossCI", "loss var rows positives")
LossCIPaired = collections.namedtuple("LossCIPaired", "loss var rows positives loss_b var_b delta var_delta")


def eval_loss_ci(pred, label, domain=None, n_domain=1, pred_b=None):
    """Log-loss with the variance of its mean per domain and over all rows; inputs as `eval_metrics` (domain: int32 [n] or a strided
    column view), pred in [0, 1].  Returns a namedtuple of device tensors with n_domain + 1 entries each — domains 0..n_domain-1,
    then ALL rows: `loss`, `var` = sum (l_i - loss)^2 / (m (m - 1)) over the segment's m per-row terms l_i (f64), `rows`,
    `positives` (i64); `loss` is `eval_metrics`' figure bit for bit.  Rows are taken as independent, as DeLong's variance takes them.
    With `pred_b` (a second prediction vector over the same rows) also `loss_b`, `var_b`, `delta` = loss - loss_b and `var_delta`,
    the variance of the PAIRED difference (formed from the rows' differences l_i(a) - l_i(b): far below var + var_b when the two
    vectors are close).  A standard error is `var.sqrt()`.  Every figure is NaN for an empty or single-class segment, as
    `eval_metrics`' loss is.  No host synchronisation; the error word (1 + a row with a NaN prediction or one outside [0, 1] in
    either vector, a label outside {0, 1} or a domain outside range) is kept as `eval_loss_ci.last_err`.
    A user-clustered error of the log-loss comes from `eval_bootstrap` with the user column as its clusters, not from here."""
    o, counts, seg, paired = _segment_ci(eval_loss_ci, "eval_loss_ci", "cdc_eval_loss_ci", pred, label, domain, n_domain, pred_b)
    if paired:
        return LossCIPaired(o[0], o[1], counts[:seg], counts[seg:], o[2], o[3], o[4], o[5])
    return LossCI(o[0], o[1], counts[:seg], counts[seg:])


GaucCI = collections.namedtuple("GaucCI", "gauc var counted left_out")
GaucCIPaired = collections.namedtuple("GaucCIPaired", "gauc var counted left_out gauc_b var_b delta var_delta")


def eval_gauc_ci(pred, label, user, n_user, domain=None, n_domain=1, user_weight=None, pred_b=None):
    """GAUC with its user-clustered variance per domain and over all rows; inputs as `eval_gauc`.  The sampling unit is the user:
    over a segment's K counted users with weight w_g and AUC A_g, `var` = K / (K - 1) * sum (w_g (A_g - gauc))^2 / (sum w_g)^2, the
    linearised variance of the ratio gauc = sum w A / sum w.  Returns a namedtuple of device tensors with n_domain + 1 entries each
    — domains 0..n_domain-1, then ALL rows: `gauc`, `var` (f64), `counted`, `left_out` (i64); `gauc` is `eval_gauc`'s figure bit
    for bit.  With `pred_b` (a second prediction vector over the same rows) also `gauc_b`, `var_b`, `delta` = gauc - gauc_b and
    `var_delta`, the variance of the PAIRED difference (the same formula on the users' differences (A_g - B_g) - delta).  A
    standard error is `var.sqrt()`.  `gauc` / `delta` are NaN where no user is counted, a variance where fewer than two are.  The
    same rows in any order give the same bits.  No host synchronisation; the error word (as `eval_gauc`'s, over both vectors) is
    kept as `eval_gauc_ci.last_err`."""
    n_user, n_domain = int(n_user), int(n_domain)
    _group_ids_ok(n_user, n_domain, n_domain + 1, "(n_domain + 1)")
    pred, label, pred_b, n = _rows("eval_gauc_ci", pred, label, pred_b)
    user, ld_user = _id_column(user, n, "user")
    domain, ld_domain, domain_p = _domain_arg(domain, n, n_domain)
    dev = pred.device
    user_weight, weight_p = _user_weight_arg(user_weight, n_user, dev)
    seg = n_domain + 1
    paired = pred_b is not None
    out = torch.empty((6 if paired else 2) * seg, dtype=torch.float64, device=dev)
    counts = torch.empty(2 * seg, dtype=torch.int64, device=dev)
    _call(eval_gauc_ci, "cdc_eval_gauc_ci", (pred.data_ptr(), _ptr(pred_b), label.data_ptr(), user.data_ptr(), ld_user, n_user, domain_p,
                                             ld_domain, n_domain, weight_p, n, out.data_ptr(), counts.data_ptr()), dev,
          ("cdc_eval_gauc_ci_workspace_bytes", n, n_domain, n_user, int(paired)),
          f"cdc_eval_gauc_ci_workspace_bytes refused n={n}, n_domain={n_domain}, n_user={n_user}")
    o = out.reshape(-1, seg)
    if paired:
        return GaucCIPaired(o[0], o[1], counts[:seg], counts[seg:], o[2], o[3], o[4], o[5])
    return GaucCI(o[0], o[1], counts[:seg], counts[seg:])


BOOT_CHUNK = 1024               # csrc/metrics.hip BOOT_CHUNK: sorted positions per workgroup of the bootstrap's passes
BOOT_REP_TILE = 8               # csrc/metrics.hip BOOT_REP_TILE: replicates a workgroup forms weights for at a time
BOOT_MAX_REP = 4096
BOOT_MAX_ROWS = (1 << 28) - 1   # 72 n^2 bounds the weighted pair count and must fit 64 bits

Bootstrap = collections.namedtuple("Bootstrap", "auc loss gauc w_rows w_pos auc_b loss_b gauc_b")


def eval_bootstrap(pred, label, cluster=None, n_cluster=None, domain=None, n_domain=1, n_rep=200, seed=0, user_weight=None, gauc=None,
                   pred_b=None):
    """Clustered bootstrap replicates of AUC, log-loss and GAUC (`cdc_eval_bootstrap`).  pred, label, domain, n_domain, user_weight,
    pred_b as `eval_gauc_ci`; `cluster` int32 [n] or a strided column view with ids in [0, n_cluster) — the user column — or None:
    then every row is its own cluster, a plain row bootstrap.  Replicate r draws ONE weight per cluster, a Poisson(1) variate capped
    at 12 that is a fixed function of (seed, r, cluster) (include/cdcmdr.h spells the hash out), and applies it to all of the
    cluster's rows: in every domain, in the "all rows" column and under both prediction vectors.  Every figure is recomputed under
    those weights, so the spread over replicates carries the correlations the analytic errors leave out: within a user, across
    domains, between two models.  `gauc`: None = when a cluster column is given.
    Returns a namedtuple `Bootstrap` of device tensors [n_rep, n_domain + 1] (domains 0..n_domain-1, then ALL rows): `auc`, `loss`,
    `gauc` (f64; gauc None when not computed), `w_rows`, `w_pos` (i64: the weighted row and positive counts), and with `pred_b` also
    `auc_b`, `loss_b`, `gauc_b` (else None) under the SAME weights: a delta's replicates are `auc - auc_b`.  auc and loss are NaN
    where a replicate leaves a segment without a class, gauc where no counted user has a positive weight.  auc does not depend on
    the row order, loss only within rounding.  At most 2^28 - 1 rows, n_rep in [1, 4096].  No host synchronisation; the error word
    (1 + a row with a NaN prediction in either vector, a label outside {0, 1}, a domain or a cluster outside range) is kept as
    `eval_bootstrap.last_err`.  `summarize_bootstrap` turns a replicate matrix into a standard error and a percentile interval.
    The calibration figures' replicates under the same weights come from `eval_calibration_bootstrap`.  Not offered: BCa or studentised
    intervals."""
    n_domain, n_rep, seed = int(n_domain), int(n_rep), int(seed)
    if n_domain <= 0:
        raise ValueError(f"n_domain={n_domain} must be positive")
    if not 1 <= n_rep <= BOOT_MAX_REP:
        raise ValueError(f"n_rep={n_rep} must lie in [1, {BOOT_MAX_REP}]")
    if not 0 <= seed < 1 << 64:
        raise ValueError(f"seed={seed} must fit 64 unsigned bits")
    if gauc is None:
        gauc = cluster is not None
    gauc = bool(gauc)
    if gauc and cluster is None:
        raise ValueError("gauc needs the cluster column: GAUC is the mean over a user's AUCs")
    if cluster is not None:
        if n_cluster is None:
            raise ValueError("a cluster column needs n_cluster, the size of the id range")
        n_cluster = int(n_cluster)
        if n_cluster <= 0:
            raise ValueError(f"n_cluster={n_cluster} must be positive")
        if gauc and (n_domain + 1) * n_cluster > 1 << 32:
            raise ValueError(f"(n_domain + 1) * n_cluster = {(n_domain + 1) * n_cluster} group ids exceed 2^32, the upper half of a sort key")
    else:
        n_cluster = 0
    pred, label, pred_b, n = _rows("eval_bootstrap", pred, label, pred_b, (BOOT_MAX_ROWS, "whose weighted pair count fits 64 bits"))
    cluster, ld_cluster, cluster_p = _id_arg(cluster, n, "cluster")
    domain, ld_domain, domain_p = _domain_arg(domain, n, n_domain)
    dev = pred.device
    user_weight, weight_p = _user_weight_arg(user_weight if gauc else None, n_cluster, dev, "clusters")
    seg = n_domain + 1
    paired = pred_b is not None
    n_stat = (3 if gauc else 2) * (2 if paired else 1)
    out = torch.empty((n_stat, n_rep, seg), dtype=torch.float64, device=dev)
    counts = torch.empty((2, n_rep, seg), dtype=torch.int64, device=dev)
    _call(eval_bootstrap, "cdc_eval_bootstrap", (pred.data_ptr(), _ptr(pred_b), label.data_ptr(), cluster_p, ld_cluster, n_cluster, domain_p,
                                                 ld_domain, n_domain, weight_p, n, n_rep, seed, int(gauc), out.data_ptr(), counts.data_ptr()),
          dev, ("cdc_eval_bootstrap_workspace_bytes", n, n_domain, n_cluster, n_rep, int(gauc)),
          f"cdc_eval_bootstrap_workspace_bytes refused n={n}, n_domain={n_domain}, n_cluster={n_cluster}, n_rep={n_rep}")
    k = 3 if gauc else 2
    return Bootstrap(out[0], out[1], out[2] if gauc else None, counts[0], counts[1], out[k] if paired else None,
                     out[k + 1] if paired else None, out[k + 2] if paired and gauc else None)


RankCI = collections.namedtuple("RankCI", "ndcg recall precision hit mrr var counted left_out reps reps_b rep_counted")
RankCIPaired = collections.namedtuple("RankCIPaired", "ndcg recall precision hit mrr var counted left_out fig_b var_b delta var_delta "
                                                      "reps reps_b rep_counted")
RANK_CI_MAX_CELLS = 1 << 20     # csrc/metrics.hip RANK_CI_MAX_CELLS: n_rep * (n_domain + 1) * len(ks)


def eval_rank_ci(pred, label, user, n_user, domain=None, n_domain=1, ks=(10,), user_weight=None, pred_b=None, n_rep=0, seed=0):
    """`eval_rank`'s figures with their user-clustered variances, the paired comparison of two prediction vectors and bootstrap
    replicates (`cdc_eval_rank_ci`).  Inputs, groups, ties and figures as `eval_rank`; `pred_b`, `n_rep` and `seed` as `eval_gauc_ci` and
    `eval_bootstrap`.  The sampling unit is the user: over a segment's G counted groups with weight w_g and value m_g,
    `var` = G / (G - 1) * sum (w_g (m_g - M))^2 / (sum w_g)^2, the linearised variance of the ratio M = sum w m / sum w.
    Returns a namedtuple of device tensors: `ndcg`, `recall`, `precision`, `hit`, `mrr` f64 [len(ks), n_domain + 1] — `eval_rank`'s
    figures bit for bit — `var` f64 [5, len(ks), n_domain + 1] in that order of figures, `counted`, `left_out` i64 [n_domain + 1].
    With `pred_b` also `fig_b`, `var_b`, `delta` = figure - fig_b and `var_delta`, the variance of the PAIRED difference (the same
    formula on the users' differences), each [5, len(ks), n_domain + 1]; identical vectors give delta = 0 and var_delta = 0 exactly.
    With `n_rep` >= 1: `reps` (and `reps_b`) f64 [n_rep, 5, len(ks), n_domain + 1], replicate r under the user weights of replicate r
    of `eval_bootstrap(seed=seed)`, NaN where no counted user has a positive weight, and `rep_counted` i64 [n_rep, n_domain + 1], the
    counted users with one; a delta's replicates are `reps - reps_b`.  Otherwise these three are None.  A figure or delta is NaN where
    no group is counted, a variance where fewer than two are.  The same rows in any order give the same bits.  n_rep in [0, 4096] and
    n_rep * (n_domain + 1) * len(ks) <= 2^20.  No host synchronisation; the error word (as `eval_rank`'s, over both vectors) is kept
    as `eval_rank_ci.last_err`."""
    n_user, n_domain, n_rep, seed = int(n_user), int(n_domain), int(n_rep), int(seed)
    _group_ids_ok(n_user, n_domain, n_domain + 1, "(n_domain + 1)")
    ks = _rank_ks(ks)
    if not 0 <= n_rep <= BOOT_MAX_REP:
        raise ValueError(f"n_rep={n_rep} must lie in [0, {BOOT_MAX_REP}]")
    if n_rep * (n_domain + 1) * len(ks) > RANK_CI_MAX_CELLS:
        raise ValueError(f"n_rep * (n_domain + 1) * len(ks) = {n_rep * (n_domain + 1) * len(ks)} cells exceed {RANK_CI_MAX_CELLS}")
    if not 0 <= seed < 1 << 64:
        raise ValueError(f"seed={seed} must fit 64 unsigned bits")
    pred, label, pred_b, n = _rows("eval_rank_ci", pred, label, pred_b)
    user, ld_user = _id_column(user, n, "user")
    domain, ld_domain, domain_p = _domain_arg(domain, n, n_domain)
    dev = pred.device
    user_weight, weight_p = _user_weight_arg(user_weight, n_user, dev)
    ks_dev, disc = _rank_ks_dev(ks, dev), rank_discounts(ks[-1], dev)
    seg, n_k, n_fig = n_domain + 1, len(ks), len(RANK_FIGURES)
    paired = pred_b is not None
    out = torch.empty((6 if paired else 2, n_fig, n_k, seg), dtype=torch.float64, device=dev)
    counts = torch.empty((2, seg), dtype=torch.int64, device=dev)
    reps = torch.empty((2 if paired else 1, n_rep, n_fig, n_k, seg), dtype=torch.float64, device=dev) if n_rep else None
    rep_counts = torch.empty((n_rep, seg), dtype=torch.int64, device=dev) if n_rep else None
    _call(eval_rank_ci, "cdc_eval_rank_ci", (pred.data_ptr(), _ptr(pred_b), label.data_ptr(), user.data_ptr(), ld_user, n_user, domain_p,
                                             ld_domain, n_domain, weight_p, ks_dev.data_ptr(), n_k, disc.data_ptr(), n, n_rep, seed,
                                             out.data_ptr(), _ptr(reps), counts.data_ptr(), _ptr(rep_counts)), dev,
          ("cdc_eval_rank_ci_workspace_bytes", n, n_domain, n_user, n_k, int(paired), n_rep),
          f"cdc_eval_rank_ci_workspace_bytes refused n={n}, n_domain={n_domain}, n_user={n_user}, n_k={n_k}, n_rep={n_rep}")
    fig = out[0]
    tail = (reps[0] if n_rep else None, reps[1] if n_rep and paired else None, rep_counts)
    if paired:
        return RankCIPaired(fig[0], fig[1], fig[2], fig[3], fig[4], out[1], counts[0], counts[1], out[2], out[3], out[4], out[5], *tail)
    return RankCI(fig[0], fig[1], fig[2], fig[3], fig[4], out[1], counts[0], counts[1], *tail)


def summarize_bootstrap(reps, level=0.95):
    """reps: a tensor [n_rep, ...] of bootstrap replicates (any device) -> (se, lo, hi, valid), each of reps' shape without its first
    axis, on the same device: `se` the standard deviation (ddof 1) over the non-NaN replicates, `lo` / `hi` the percentile interval
    at (1 -+ level) / 2 (`torch.nanquantile`, linear interpolation), `valid` (i64) the count of non-NaN replicates; se, lo and hi
    are NaN where valid < 2.  No host synchronisation."""
    if not 0.0 < float(level) < 1.0:
        raise ValueError(f"level={level} must lie in (0, 1)")
    reps = reps.to(torch.float64)
    ok = ~torch.isnan(reps)
    valid = ok.sum(0)
    cnt = valid.to(torch.float64)
    zero = torch.zeros((), dtype=torch.float64, device=reps.device)
    mean = torch.where(ok, reps, zero).sum(0) / cnt
    dev2 = torch.where(ok, (reps - mean) ** 2, zero).sum(0)
    se = (dev2 / (cnt - 1)).sqrt()
    q = torch.tensor([(1.0 - level) / 2, (1.0 + level) / 2], dtype=torch.float64, device=reps.device)
    lo, hi = torch.nanquantile(reps, q, dim=0)
    few = valid < 2
    nan = torch.full((), math.nan, dtype=torch.float64, device=reps.device)
    return torch.where(few, nan, se), torch.where(few, nan, lo), torch.where(few, nan, hi), valid


Calibration = collections.namedtuple("Calibration", "rows positives mean_pred ctr pcoc brier ece mce ece_q mce_q table table_q")
CalibrationTable = collections.namedtuple("CalibrationTable", "count positives mean_pred pos_rate pred_min pred_max")
MAX_CALIBRATION_BINS = 1024


def eval_calibration(pred, label, domain=None, n_domain=1, n_bins=10):
    """Calibration of probabilities per domain and over all rows; inputs as `eval_metrics` (domain: int32 [n] or a strided column
    view), pred in [0, 1], 1 <= n_bins <= 1024.  A prediction enters every sum as the integer q = rint(p * 2^32), so the sums are
    exact and the same rows in any order give the same bits.  Returns a namedtuple of device tensors.  Per segment (n_domain + 1
    entries: domains 0..n_domain-1, then ALL rows): `rows`, `positives` (i64), `mean_pred`, `ctr`, `pcoc` = predicted over observed
    CTR (NaN without positives), `brier`, and the expected / maximum calibration error over n_bins equal-width bins (`ece`, `mce`:
    a row is in bin min(n_bins-1, floor(p * n_bins))) and over n_bins equal-mass bins (`ece_q`, `mce_q`: bin b holds the sorted
    positions [floor(b m / n_bins), floor((b+1) m / n_bins)) of the segment's m rows in (score, label) order), all f64 and NaN for a
    segment without rows.  `table` / `table_q`: the two reliability tables, namedtuples (count, positives i64; mean_pred, pos_rate
    f64; pred_min, pred_max f32) of shape [n_domain + 1, n_bins]; an empty bin has count 0 and NaN in the floating-point fields.
    No host synchronisation; the error word (1 + a row with a NaN prediction, a prediction outside [0, 1], a label outside {0, 1} or
    a domain outside range) is kept as `eval_calibration.last_err`.
    A recalibration map is fitted by `eval_isotonic_fit` / `Recalibration` (isotonic regression) or `eval_platt_fit` /
    `PlattRecalibration` (Platt, temperature, bias scaling); `eval_calibration_bootstrap` gives pcoc, brier, ece and ece_q their
    bootstrap intervals, `Evaluator(calibration_ci=True)` reports them and the calibration deltas of `Evaluator.compare`.  Not
    offered: selection or early stopping by a calibration figure in `Runner`."""
    n_domain, n_bins = int(n_domain), int(n_bins)
    if not 1 <= n_bins <= MAX_CALIBRATION_BINS:
        raise ValueError(f"n_bins={n_bins} must lie in [1, {MAX_CALIBRATION_BINS}]")
    pred, label, _, n = _rows("eval_calibration", pred, label)
    domain, ld, domain_p = _domain_arg(domain, n, n_domain)
    dev = pred.device
    seg = n_domain + 1
    seg_out = torch.empty((8, seg), dtype=torch.float64, device=dev)
    seg_counts = torch.empty((2, seg), dtype=torch.int64, device=dev)
    tab_out = torch.empty((2, 2, seg, n_bins), dtype=torch.float64, device=dev)
    tab_counts = torch.empty((2, 2, seg, n_bins), dtype=torch.int64, device=dev)
    tab_range = torch.empty((2, 2, seg, n_bins), dtype=torch.float32, device=dev)
    _call(eval_calibration, "cdc_eval_calibration", (pred.data_ptr(), label.data_ptr(), domain_p, ld, n, n_domain, n_bins, seg_out.data_ptr(),
                                                     seg_counts.data_ptr(), tab_out.data_ptr(), tab_counts.data_ptr(), tab_range.data_ptr()),
          dev, ("cdc_eval_calibration_workspace_bytes", n, n_domain, n_bins),
          f"cdc_eval_calibration_workspace_bytes refused n={n}, n_domain={n_domain}, n_bins={n_bins}")
    tables = [CalibrationTable(tab_counts[t, 0], tab_counts[t, 1], tab_out[t, 0], tab_out[t, 1], tab_range[t, 0], tab_range[t, 1]) for t in (0, 1)]
    return Calibration(seg_counts[0], seg_counts[1], *seg_out.unbind(0), tables[0], tables[1])


CALBOOT_CHUNK = 1024            # csrc/metrics.hip CALBOOT_CHUNK: sorted positions per workgroup of the calibration bootstrap's passes
CALBOOT_REP_TILE = 8            # csrc/metrics.hip CALBOOT_REP_TILE: replicates whose weights a lane holds at a time
CALBOOT_MAX_CELLS = 1 << 22     # csrc/metrics.hip CALBOOT_MAX_CELLS: n_rep * (n_domain + 1) * n_bins

CalibrationBootstrap = collections.namedtuple("CalibrationBootstrap", "pcoc brier ece ece_q w_rows w_pos pcoc_b brier_b ece_b ece_q_b")


def eval_calibration_bootstrap(pred, label, cluster=None, n_cluster=None, domain=None, n_domain=1, n_bins=10, n_rep=200, seed=0,
                               pred_b=None):
    """Clustered bootstrap replicates of the calibration figures (`cdc_eval_calibration_bootstrap`).  pred, label, domain, n_domain,
    n_bins as `eval_calibration`; cluster, n_cluster, n_rep, seed, pred_b as `eval_bootstrap`: replicate r gives every row the weight
    `eval_bootstrap` gives it for the same (seed, r, cluster) — rows are their own clusters without a cluster column — and a
    replicate's figures are BY DEFINITION `eval_calibration`'s on the rows repeated by their weights: pcoc, brier, ece over the
    equal-width bins (a row's bin depends on its prediction alone) and ece_q over equal-mass bins of the REPEATED rows (a row's
    copies may fall into several bins).  Returns the namedtuple `CalibrationBootstrap` of device tensors [n_rep, n_domain + 1]
    (domains 0..n_domain-1, then ALL rows): `pcoc`, `brier`, `ece`, `ece_q` (f64), `w_rows`, `w_pos` (i64: the weighted row and
    positive counts, `eval_bootstrap`'s integers), and with `pred_b` also `pcoc_b`, `brier_b`, `ece_b`, `ece_q_b` (else None) under
    the SAME weights: a delta's replicates are `ece - ece_b`.  Every figure is NaN where a replicate leaves a segment without rows,
    pcoc also where it leaves it without positives; a single-class segment still has brier and ece.  All sums are exact integers:
    the same rows in any order give the same bits, and a replicate equals `eval_calibration` on the repeated rows bit for bit.  At
    most 2^28 - 1 rows, n_rep in [1, 4096], n_rep * (n_domain + 1) * n_bins <= 2^22 cells.  No host synchronisation; the error word
    (1 + a row with a prediction outside [0, 1] or NaN in either vector, a label outside {0, 1}, a domain or a cluster outside
    range; the row is counted clamped) is kept as `eval_calibration_bootstrap.last_err`.  `summarize_bootstrap` applies unchanged.
    ECE is biased upwards on small segments, replicates included: the interval of a delta is more trustworthy than that of a level.
    Not offered: MCE replicates, per-bin reliability bands, BCa or studentised intervals, selection by a calibration figure in
    `Runner`."""
    n_domain, n_bins, n_rep, seed = int(n_domain), int(n_bins), int(n_rep), int(seed)
    if n_domain <= 0:
        raise ValueError(f"n_domain={n_domain} must be positive")
    if not 1 <= n_bins <= MAX_CALIBRATION_BINS:
        raise ValueError(f"n_bins={n_bins} must lie in [1, {MAX_CALIBRATION_BINS}]")
    if not 1 <= n_rep <= BOOT_MAX_REP:
        raise ValueError(f"n_rep={n_rep} must lie in [1, {BOOT_MAX_REP}]")
    if not 0 <= seed < 1 << 64:
        raise ValueError(f"seed={seed} must fit 64 unsigned bits")
    if n_rep * (n_domain + 1) * n_bins > CALBOOT_MAX_CELLS:
        raise ValueError(f"n_rep * (n_domain + 1) * n_bins = {n_rep * (n_domain + 1) * n_bins} cells exceed the cell cap "
                         f"CALBOOT_MAX_CELLS = {CALBOOT_MAX_CELLS}")
    if cluster is not None:
        if n_cluster is None:
            raise ValueError("a cluster column needs n_cluster, the size of the id range")
        n_cluster = int(n_cluster)
        if n_cluster <= 0:
            raise ValueError(f"n_cluster={n_cluster} must be positive")
    else:
        n_cluster = 0
    pred, label, pred_b, n = _rows("eval_calibration_bootstrap", pred, label, pred_b, (BOOT_MAX_ROWS, "whose weighted sums fit 64 bits"))
    cluster, ld_cluster, cluster_p = _id_arg(cluster, n, "cluster")
    domain, ld_domain, domain_p = _domain_arg(domain, n, n_domain)
    dev = pred.device
    seg = n_domain + 1
    paired = pred_b is not None
    out = torch.empty((8 if paired else 4, n_rep, seg), dtype=torch.float64, device=dev)
    counts = torch.empty((2, n_rep, seg), dtype=torch.int64, device=dev)
    _call(eval_calibration_bootstrap, "cdc_eval_calibration_bootstrap",
          (pred.data_ptr(), _ptr(pred_b), label.data_ptr(), cluster_p, ld_cluster, n_cluster, domain_p, ld_domain, n_domain, n_bins, n, n_rep,
           seed, out.data_ptr(), counts.data_ptr()), dev, ("cdc_eval_calibration_bootstrap_workspace_bytes", n, n_domain, n_bins, n_rep, int(paired)),
          f"cdc_eval_calibration_bootstrap_workspace_bytes refused n={n}, n_domain={n_domain}, n_bins={n_bins}, n_rep={n_rep}")
    second = tuple(out[4:]) if paired else (None,) * 4
    return CalibrationBootstrap(out[0], out[1], out[2], out[3], counts[0], counts[1], *second)


IsotonicFit = collections.namedtuple("IsotonicFit", "start x_lo x_hi count positives value rows seg_positives")


def eval_isotonic_fit(pred, label, domain=None, n_domain=1):
    """Isotonic regression of the labels on the score per domain and over all rows; inputs as `eval_metrics` (domain: int32 [n] or a
    strided column view), pred any finite float32 (logits are allowed; -0.0 and +0.0 are one score).  Returns the namedtuple
    `IsotonicFit` of device tensors: `start` i64 [n_domain + 2] — the blocks of segment s (domains 0..n_domain-1, then ALL rows) are
    [start[s], start[s+1]) — and per block, in ascending score order, `x_lo`, `x_hi` (f32: its smallest and largest score), `count`,
    `positives` (i64) and `value` = positives / count (f64), strictly increasing along a segment; `rows`, `seg_positives` i64
    [n_domain + 1].  The block tensors have the full capacity 2n, entries at or past start[-1] are not written.  The fit is exact
    (integer comparisons until the one division), so the same rows in any order give the same bits.  No host synchronisation; the
    error word (1 + a row with a NaN or infinite score, a label outside {0, 1} or a domain outside range) is kept as
    `eval_isotonic_fit.last_err`."""
    n_domain = int(n_domain)
    pred, label, _, n = _rows("eval_isotonic_fit", pred, label)
    domain, ld, domain_p = _domain_arg(domain, n, n_domain)
    dev = pred.device
    seg = n_domain + 1
    refused = f"cdc_eval_isotonic_fit_workspace_bytes refused n={n}, n_domain={n_domain}"
    cap = L.load().cdc_eval_isotonic_max_blocks(n, n_domain)
    if cap <= 0:
        raise RuntimeError(refused)
    start = torch.empty(seg + 1, dtype=torch.int64, device=dev)
    x = torch.empty((2, cap), dtype=torch.float32, device=dev)
    cnt = torch.empty((2, cap), dtype=torch.int64, device=dev)
    value = torch.empty(cap, dtype=torch.float64, device=dev)
    seg_counts = torch.empty((2, seg), dtype=torch.int64, device=dev)
    _call(eval_isotonic_fit, "cdc_eval_isotonic_fit", (pred.data_ptr(), label.data_ptr(), domain_p, ld, n, n_domain, start.data_ptr(),
                                                       x[0].data_ptr(), x[1].data_ptr(), cnt[0].data_ptr(), cnt[1].data_ptr(), value.data_ptr(),
                                                       cap, seg_counts[0].data_ptr(), seg_counts[1].data_ptr()), dev,
          ("cdc_eval_isotonic_fit_workspace_bytes", n, n_domain), refused)
    return IsotonicFit(start, x[0], x[1], cnt[0], cnt[1], value, seg_counts[0], seg_counts[1])


def eval_isotonic_apply(pred, fit_or_map, domain=None, n_domain=1, seg_of_domain=None, eps=0.0):
    """The isotonic map of `fit_or_map` (an `IsotonicFit` or a `Recalibration`) at the scores pred f32 [n]: a row of domain d goes
    through the blocks of segment seg_of_domain[d] (int32 [n_domain], entries in [0, n_domain]; None: the identity, or the
    `Recalibration`'s own table) — constant on a block, linear between two blocks, the first / last value outside; float64
    arithmetic, the result float32, clamped to [eps, 1 - eps] when eps > 0.  Returns float32 [n] on the device.  A NaN score, a domain
    outside range or a segment without blocks gives NaN and sets the error word (1 + the row), kept as
    `eval_isotonic_apply.last_err`.  No host synchronisation.  Not offered: a "step" interpolation (the parametric maps are
    `eval_platt_fit` / `eval_platt_apply`)."""
    n_domain = int(n_domain)
    pred, _, _, n = _rows("eval_isotonic_apply", pred)
    domain, ld, domain_p = _domain_arg(domain, n, n_domain)
    dev = pred.device
    m = fit_or_map
    if m.start.numel() != n_domain + 2:
        raise ValueError(f"the map holds {m.start.numel() - 2} domains, not {n_domain}")
    if seg_of_domain is None:
        seg_of_domain = getattr(m, "seg_of_domain", None)
    if seg_of_domain is None:
        seg_of_domain = torch.arange(n_domain, dtype=torch.int32, device=dev)
    seg_of_domain = torch.as_tensor(seg_of_domain).to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
    if seg_of_domain.numel() != n_domain:
        raise ValueError(f"seg_of_domain holds {seg_of_domain.numel()} entries for {n_domain} domains")
    if not 0.0 <= float(eps) <= 0.5:
        raise ValueError(f"eps={eps} must lie in [0, 0.5]")
    out = torch.empty(n, dtype=torch.float32, device=dev)
    _call(eval_isotonic_apply, "cdc_eval_isotonic_apply", (pred.data_ptr(), domain_p, ld, n, n_domain, seg_of_domain.data_ptr(),
                                                           m.start.data_ptr(), m.x_lo.data_ptr(), m.x_hi.data_ptr(), m.value.data_ptr(),
                                                           float(eps), out.data_ptr()), dev)
    return out


IsotonicBlocks = collections.namedtuple("IsotonicBlocks", "x_lo x_hi count positives value")


class Recalibration:
    """A fitted per-domain isotonic map: the blocks of `eval_isotonic_fit` cut to their number, and `seg_of_domain`, the segment
    every domain is sent through — its own, or "all" (index n_domain) for the domains of `fallback_domains`."""
    _TENSORS = ("start", "x_lo", "x_hi", "count", "positives", "value", "rows", "seg_positives", "seg_of_domain")

    def __init__(self):
        self.n_domain = 0
        self.fallback_domains = []
        for k in self._TENSORS:
            setattr(self, k, None)

    @classmethod
    def fit(cls, pred, label, domain=None, n_domain=1, min_rows=0, need_both_classes=True):
        """Fits on (pred, label, domain) — the validation split's RAW predictions.  A domain without fit rows, with fewer than
        min_rows, or (need_both_classes) with a single class has no map of its own worth using: it is sent through the map of all
        rows and listed in `fallback_domains`.  One host synchronisation: start, rows, seg_positives and the error word are read
        once.  A bad row (non-finite score, label outside {0, 1}, domain outside range) raises ValueError naming it."""
        n_domain = int(n_domain)
        f = eval_isotonic_fit(pred, label, domain, n_domain)
        seg = n_domain + 1
        host = torch.cat([f.start, f.rows, f.seg_positives, eval_isotonic_fit.last_err.to(torch.int64)]).cpu().tolist()   # the one sync
        start, rows, pos, bad = host[:seg + 1], host[seg + 1:2 * seg + 1], host[2 * seg + 1:3 * seg + 1], host[-1]
        if bad:
            raise ValueError(f"recalibration row {bad - 1}: NaN or infinite score, label outside {{0,1}} or domain outside [0, {n_domain})")
        r = cls()
        r.n_domain = n_domain
        nb = start[seg]
        r.start, r.rows, r.seg_positives = f.start, f.rows, f.seg_positives
        for k in ("x_lo", "x_hi", "count", "positives", "value"):
            setattr(r, k, getattr(f, k)[:nb].clone())              # the full-capacity buffers go
        r.fallback_domains = [d for d in range(n_domain)
                              if rows[d] == 0 or rows[d] < min_rows or (need_both_classes and (pos[d] == 0 or pos[d] == rows[d]))]
        table = [n_domain if d in set(r.fallback_domains) else d for d in range(n_domain)]
        r.seg_of_domain = torch.tensor(table, dtype=torch.int32, device=f.start.device)
        return r

    def apply(self, pred, domain=None, eps=0.0):
        """-> float32 [n] on the device: pred through the map of every row's domain (domain: as `eval_metrics`; None for a map over
        one domain)."""
        return eval_isotonic_apply(pred, self, domain, self.n_domain, self.seg_of_domain, eps)

    def state_dict(self):
        sd = {k: getattr(self, k) for k in self._TENSORS}
        sd["fallback_domains"] = torch.tensor(self.fallback_domains, dtype=torch.int64)
        return sd

    def load_state_dict(self, sd, device=None):
        for k in self._TENSORS:
            t = sd[k]
            setattr(self, k, t.to(device) if device is not None else t)
        self.n_domain = self.seg_of_domain.numel()
        self.fallback_domains = [int(d) for d in sd["fallback_domains"].tolist()]
        return self

    def blocks(self, segment):
        """Host numpy arrays (x_lo, x_hi, count, positives, value) of a domain's own blocks, or of "all" (also: index n_domain)."""
        s = self.n_domain if segment == "all" else int(segment)
        if not 0 <= s <= self.n_domain:
            raise ValueError(f"segment {segment!r} outside [0, {self.n_domain}] / 'all'")
        b0, b1 = self.start[s:s + 2].cpu().tolist()
        return IsotonicBlocks(*(getattr(self, k)[b0:b1].cpu().numpy() for k in IsotonicBlocks._fields))


PlattFit = collections.namedtuple("PlattFit", "a b rows positives loss_before loss_after grad iterations status")
PLATT_METHODS = {"platt": 0, "temperature": 1, "bias": 2}
PLATT_INPUTS = {"prob": 0, "logit": 1}
PLATT_CONVERGED, PLATT_EMPTY, PLATT_SLOPE_FIXED = 1, 2, 4


def _platt_args(method, input, clip):
    if method is not None and method not in PLATT_METHODS:
        raise ValueError(f"method={method!r} is none of {sorted(PLATT_METHODS)}")
    if input not in PLATT_INPUTS:
        raise ValueError(f"input={input!r} is none of {sorted(PLATT_INPUTS)}")
    if not 1e-12 <= float(clip) <= 0.25:
        raise ValueError(f"clip={clip} must lie in [1e-12, 0.25]")


def eval_platt_fit(pred, label, domain=None, n_domain=1, method="platt", input="prob", clip=1e-7, gtol=1e-10, max_iter=32):
    """Platt scaling per domain and over all rows: the map sigmoid(a z + b) of the logit-scale score z that minimises the
    cross-entropy against Platt's smoothed targets (P + 1) / (P + 2) and 1 / (N + 2); inputs as `eval_metrics`.  input "prob":
    pred in [0, 1], z = log(p) - log1p(-p); "logit": z = pred; both clamped to +-log((1 - clip) / clip).  method "platt": a and b;
    "temperature": a alone (b = 0); "bias": b alone (a = 1) — the exact repair of negative down-sampling.  Newton steps with a
    backtracking line search from (1, 0) on the device, until the mean gradient's inf-norm is <= gtol or max_iter steps are spent.
    Returns the namedtuple `PlattFit` of device tensors with n_domain + 1 entries (domains, then ALL rows): a, b (f64), rows,
    positives (i64), loss_before, loss_after (the plain mean BCE of sigmoid(z) and of the map), grad (f64), iterations, status (i32:
    PLATT_CONVERGED | PLATT_EMPTY | PLATT_SLOPE_FIXED — "platt" on a segment with a single z fits b alone).  The same rows in any
    order give the same bits.  No host synchronisation; the error word (1 + a row with a NaN score, a probability outside [0, 1], a
    label outside {0, 1} or a domain outside range; such a row counts with z = 0 and label 0) is kept as `eval_platt_fit.last_err`.
    Not offered: beta calibration, vector or matrix scaling."""
    n_domain, max_iter = int(n_domain), int(max_iter)
    _need_device("eval_platt_fit", pred)                                   # before the option checks, as ever
    _platt_args(method, input, clip)
    if not float(gtol) > 0.0:
        raise ValueError(f"gtol={gtol} must be positive")
    if not 1 <= max_iter <= 1024:
        raise ValueError(f"max_iter={max_iter} must lie in [1, 1024]")
    pred, label, _, n = _rows("eval_platt_fit", pred, label)
    domain, ld, domain_p = _domain_arg(domain, n, n_domain)
    dev = pred.device
    seg = n_domain + 1
    f64 = torch.empty((5, seg), dtype=torch.float64, device=dev)
    i64 = torch.empty((2, seg), dtype=torch.int64, device=dev)
    i32 = torch.empty((2, seg), dtype=torch.int32, device=dev)
    _call(eval_platt_fit, "cdc_eval_platt_fit", (pred.data_ptr(), label.data_ptr(), domain_p, ld, n, n_domain, PLATT_METHODS[method],
                                                 PLATT_INPUTS[input], float(clip), float(gtol), max_iter, f64[0].data_ptr(), f64[1].data_ptr(),
                                                 f64[2].data_ptr(), f64[3].data_ptr(), f64[4].data_ptr(), i64[0].data_ptr(), i64[1].data_ptr(),
                                                 i32[0].data_ptr(), i32[1].data_ptr()), dev, ("cdc_eval_platt_fit_workspace_bytes", n, n_domain),
          f"cdc_eval_platt_fit_workspace_bytes refused n={n}, n_domain={n_domain}")
    return PlattFit(f64[0], f64[1], i64[0], i64[1], f64[2], f64[3], f64[4], i32[0], i32[1])


def eval_platt_apply(pred, fit_or_map, domain=None, n_domain=1, seg_of_domain=None, input="prob", clip=1e-7, eps=0.0):
    """The map of `fit_or_map` (a `PlattFit` or a `PlattRecalibration`) at the scores pred f32 [n]: a row of domain d gets
    sigmoid(a[s] z + b[s]) with s = seg_of_domain[d] (int32 [n_domain], entries in [0, n_domain]; None: the identity, or the
    `PlattRecalibration`'s own table) and z as in `eval_platt_fit` — give the fit's `input` and `clip`; float64 arithmetic, the result
    float32, clamped to [eps, 1 - eps] when eps > 0.  Returns float32 [n] on the device.  A NaN score, a probability outside [0, 1]
    or a domain outside range gives NaN and sets the error word (1 + the row), kept as `eval_platt_apply.last_err`.  No host
    synchronisation."""
    n_domain = int(n_domain)
    _need_device("eval_platt_apply", pred)                                 # before the option checks, as ever
    _platt_args(None, input, clip)
    pred, _, _, n = _rows("eval_platt_apply", pred)
    domain, ld, domain_p = _domain_arg(domain, n, n_domain)
    dev = pred.device
    m = fit_or_map
    if m.a.numel() != n_domain + 1:
        raise ValueError(f"the map holds {m.a.numel() - 1} domains, not {n_domain}")
    if seg_of_domain is None:
        seg_of_domain = getattr(m, "seg_of_domain", None)
    if seg_of_domain is None:
        seg_of_domain = torch.arange(n_domain, dtype=torch.int32, device=dev)
    seg_of_domain = torch.as_tensor(seg_of_domain).to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
    if seg_of_domain.numel() != n_domain:
        raise ValueError(f"seg_of_domain holds {seg_of_domain.numel()} entries for {n_domain} domains")
    if not 0.0 <= float(eps) <= 0.5:
        raise ValueError(f"eps={eps} must lie in [0, 0.5]")
    a = m.a.to(device=dev, dtype=torch.float64).contiguous()
    b = m.b.to(device=dev, dtype=torch.float64).contiguous()
    out = torch.empty(n, dtype=torch.float32, device=dev)
    _call(eval_platt_apply, "cdc_eval_platt_apply", (pred.data_ptr(), domain_p, ld, n, n_domain, seg_of_domain.data_ptr(), a.data_ptr(),
                                                     b.data_ptr(), PLATT_INPUTS[input], float(clip), float(eps), out.data_ptr()), dev)
    return out


class PlattRecalibration:
    """A fitted per-domain map sigmoid(a z + b) (`eval_platt_fit`) and `seg_of_domain`, the segment every domain is sent through —
    its own, or "all" (index n_domain) for the domains of `fallback_domains`.  The surface `Evaluator` uses is `Recalibration`'s."""
    _TENSORS = ("a", "b", "rows", "positives", "loss_before", "loss_after", "grad", "iterations", "status", "seg_of_domain")

    def __init__(self):
        self.n_domain = 0
        self.fallback_domains = []
        self.method, self.input, self.clip = "platt", "prob", 1e-7
        for k in self._TENSORS:
            setattr(self, k, None)

    @classmethod
    def fit(cls, pred, label, domain=None, n_domain=1, method="platt", input="prob", clip=1e-7, gtol=1e-10, max_iter=32, min_rows=0,
            need_both_classes=True, need_increasing=True):
        """Fits on (pred, label, domain) — the validation split's RAW predictions.  A domain without fit rows, with fewer than
        min_rows, (need_both_classes) with a single class, whose fit did not converge, or (need_increasing) with a <= 0 is sent
        through the map of all rows and listed in `fallback_domains`.  One host synchronisation: a, rows, positives, status and the
        error word are read once.  A bad row (NaN score, probability outside [0, 1], label outside {0, 1}, domain outside range)
        raises ValueError naming it."""
        n_domain = int(n_domain)
        f = eval_platt_fit(pred, label, domain, n_domain, method, input, clip, gtol, max_iter)
        seg = n_domain + 1
        host = torch.cat([f.a, f.rows.to(torch.float64), f.positives.to(torch.float64), f.status.to(torch.float64),
                          eval_platt_fit.last_err.to(torch.float64)]).cpu().tolist()                  # the one sync; counts < 2^53
        a, rows, pos, status, bad = host[:seg], host[seg:2 * seg], host[2 * seg:3 * seg], host[3 * seg:4 * seg], int(host[-1])
        if bad:
            raise ValueError(f"recalibration row {bad - 1}: NaN score, probability outside [0, 1], label outside {{0,1}} or domain "
                             f"outside [0, {n_domain})")
        r = cls()
        r.n_domain, r.method, r.input, r.clip = n_domain, method, input, float(clip)
        for k in PlattFit._fields:
            setattr(r, k, getattr(f, k))
        r.fallback_domains = [d for d in range(n_domain)
                              if rows[d] == 0 or rows[d] < min_rows or (need_both_classes and (pos[d] == 0 or pos[d] == rows[d]))
                              or not int(status[d]) & PLATT_CONVERGED or (need_increasing and not a[d] > 0.0)]
        back = set(r.fallback_domains)
        r.seg_of_domain = torch.tensor([n_domain if d in back else d for d in range(n_domain)], dtype=torch.int32, device=f.a.device)
        return r

    def apply(self, pred, domain=None, eps=0.0):
        """-> float32 [n] on the device: pred through the map of every row's domain (domain: as `eval_metrics`; None for a map over
        one domain)."""
        return eval_platt_apply(pred, self, domain, self.n_domain, self.seg_of_domain, self.input, self.clip, eps)

    def params(self, segment):
        """Host (a, b, status) of a domain's own fit, or of "all" (also: index n_domain)."""
        s = self.n_domain if segment == "all" else int(segment)
        if not 0 <= s <= self.n_domain:
            raise ValueError(f"segment {segment!r} outside [0, {self.n_domain}] / 'all'")
        return float(self.a[s].item()), float(self.b[s].item()), int(self.status[s].item())

    def state_dict(self):
        sd = {k: getattr(self, k) for k in self._TENSORS}
        sd["fallback_domains"] = torch.tensor(self.fallback_domains, dtype=torch.int64)
        sd["method"] = torch.tensor(PLATT_METHODS[self.method], dtype=torch.int64)
        sd["input"] = torch.tensor(PLATT_INPUTS[self.input], dtype=torch.int64)
        sd["clip"] = torch.tensor(self.clip, dtype=torch.float64)
        return sd

    def load_state_dict(self, sd, device=None):
        for k in self._TENSORS:
            t = sd[k]
            setattr(self, k, t.to(device) if device is not None else t)
        self.n_domain = self.seg_of_domain.numel()
        self.fallback_domains = [int(d) for d in sd["fallback_domains"].tolist()]
        self.method = {v: k for k, v in PLATT_METHODS.items()}[int(sd["method"])]
        self.input = {v: k for k, v in PLATT_INPUTS.items()}[int(sd["input"])]
        self.clip = float(sd["clip"])
        return self


def _se(var):
    return math.sqrt(var) if var == var else math.nan


def _z(delta, se):
    """delta / se; NaN for 0 / 0, +-inf for a non-zero delta over se 0"""
    if se != se or delta != delta:
        return math.nan
    if se == 0:
        return math.nan if delta == 0 else math.copysign(math.inf, delta)
    return delta / se


class Evaluator:
    """Mirror of Run.test (run.py:647-690): the CDC, multi-tower and single-tower branches.

    mode "cdc": `data_loader` is ({domain: loader of (X, y)}, domain_batch_seq) as data.make_domain_loaders returns them for the
                validation / test split; for every d of the sequence the next batch of domain d is scored by the tower of d's
                group: pred = model(X, mode='split', domain_i=d)                       (run.py:653-661, get_domain_data 499-526)
    mode "multi": batches are (X, y, group) and pred = model(X).gather(1, group)   (run.py:668-673)
    mode "single": batches are (X, y) and pred = model(X)                           (run.py:674-676)
    domain_cnt_weight: {domain: weight} or a sequence, as Run.domain_cnt_weight (mean_auc / mean_loss, run.py:706-707).
    user_idx: column of X that holds the user id (in [0, n_user)).  When set, test() adds GAUC (base.py:33-64): total_gauc, and
              with per-domain evaluation domain_gauc and mean_gauc.  user_weight: f64 [n_user] or {user: weight} (a user missing
              from the dict weighs NaN: the reference raises KeyError for it), None = the user's row count.
    auc_ci: test() adds the DeLong standard errors of its AUCs (`eval_auc_ci`): total_auc_se, and with per-domain evaluation
            domain_auc_se {d: value} and mean_auc_se = sqrt(sum_d w_d^2 var_d) over the domains mean_auc sums (disjoint row sets:
            independent given the model).
    loss_ci: test() adds the standard errors of its log-losses (`eval_loss_ci`; rows taken as independent): total_loss_se, and with
            per-domain evaluation domain_loss_se {d: value} and mean_loss_se = sqrt(sum_d w_d^2 var_d), as mean_auc_se; compare()
            adds total_loss_delta = loss(self) - loss(other), total_loss_delta_se (from the rows' paired differences) and
            total_loss_z, and the domain_loss_* / mean_loss_* forms.
    gauc_ci: (needs user_idx) test() adds the user-clustered standard errors of its GAUCs (`eval_gauc_ci`): total_gauc_se, and with
            per-domain evaluation domain_gauc_se {d: value}.  mean_gauc_se is NOT offered: a user's rows span domains, so the
            per-domain GAUCs are not independent and sqrt(sum_d w_d^2 var_d) would not be their mean's standard error.  compare()
            adds total_gauc_delta, total_gauc_delta_se, total_gauc_z and the domain_gauc_* forms.
            mean_gauc's error and a user-clustered error of the log-loss come from `bootstrap` (mean_gauc_boot_se, *_loss_boot_se).
    bootstrap: None (off: the result dictionaries and launches are exactly those without it) or the number of replicates of a
            clustered bootstrap (`eval_bootstrap`; seed `bootstrap_seed`, interval level `bootstrap_level`).  Clusters are the users
            when user_idx is set, otherwise rows.  test() adds, for auc and loss and with user_idx for gauc, total_*_boot_se,
            total_*_boot_lo, total_*_boot_hi (standard deviation and percentile interval over the replicates) and with per-domain
            evaluation domain_*_boot_se/lo/hi {d: value} and mean_*_boot_se/lo/hi — the mean formed PER REPLICATE, sum over the
            present domains of weight(d) * figure_d, so mean_gauc_boot_se is valid where mean_gauc_se cannot be offered; a replicate
            in which a present domain is NaN is left out of the mean's summary.  boot_valid is the smallest number of non-NaN
            replicates behind any reported figure.  compare() adds total_delta_boot_se/lo/hi (+ domain_ / mean_ forms), with loss_ci
            the *_loss_delta_boot_* forms and with gauc_ci the *_gauc_delta_boot_* forms (mean_gauc_delta_boot_* included), all from
            per-replicate differences under shared weights.  The bootstrap launches are queued with the others, before the one
            synchronisation.
            Not offered: significance-aware early stopping in `Runner`, BCa or studentised intervals.
    rank_at: None (off: the result dictionaries and launches are exactly those without it), an int or a tuple of ints (needs user_idx):
            the cut-offs K of the per-user top-K figures (`eval_rank`: up to 8 strictly increasing values in [1, 1024]).  test() adds,
            for fig in ndcg, recall, precision, hit, mrr and every K, total_<fig>@<K>, and with per-domain evaluation domain_<fig>@<K>
            {d: value} and mean_<fig>@<K>, weighted like mean_gauc (NaN when a present domain counts no user), and total_rank_users
            (+ domain_rank_users): the users with at least one positive, over whom the figures are averaged — with user_weight when one
            was given, uniformly otherwise (GAUC's default is the row count).  The launch is queued with the others, before the one
            synchronisation.  Standard errors, bootstrap intervals and `compare` deltas come with `rank_ci`.  Not offered: graded gains,
            sampled-negative protocols, MAP.
    rank_ci: (needs rank_at, and hence user_idx; ValueError otherwise) the user-clustered standard errors of the top-K figures
            (`eval_rank_ci`, one call in place of `eval_rank`'s: the total_/domain_/mean_<fig>@<K> keys keep their bits).  test() adds
            total_<fig>@<K>_se and with per-domain evaluation domain_<fig>@<K>_se {d: value}; no mean_<fig>@<K>_se, for mean_gauc_se's
            reason: a user's rows span domains.  With bootstrap also total_/domain_/mean_<fig>@<K>_boot_se/lo/hi from the same call's
            replicates (the evaluator's replicate count, seed and level; the mean formed per replicate under mean_<fig>@<K>'s weights);
            boot_valid covers them.  compare() adds total_<fig>@<K>_delta, _delta_se and _z and the domain_ forms, and with bootstrap
            the *_delta_boot_se/lo/hi forms, mean_<fig>@<K>_delta, mean_<fig>@<K>_delta_boot_* and mean_<fig>@<K>_z = delta / boot_se —
            then both passes must see the same user column.  Without it every result dictionary and every launch is exactly as
            before.  Not offered: BCa or studentised intervals, significance-aware early stopping in `Runner`.
    recommend(loader, k, item_idx, by): (a method, needs user_idx; no constructor argument, test() and compare() are untouched) the
            per-user top-K lists themselves (`eval_topk`): one scoring pass, recalibrated like predict(), -> a `TopK` with every
            (domain, user) group's — by="user": every user's — k best rows, best first, no item of column item_idx twice, and the
            entries' labels.  Not offered: graded relevance, diversity or business re-ranking, lists under data parallelism.
    recommend_catalog(context, catalog, item_cols, k, seen, domain2group, tile_rows, item_block): (a method; no constructor argument)
            every context's k best items out of a catalogue (`catalog_rows`, `catalog_topk`: the user x item pool written, scored
            and ranked tile by tile) -> a `CatalogTopK`.  Not offered: grouping of contexts by user, graded relevance, diversity
            re-ranking, data parallelism, a survivor count before the cut.
    calibration: test() adds calibration figures (`eval_calibration`; True: 10 bins, an int: that many): total_pcoc (predicted over
            observed CTR), total_brier, total_ece, total_ece_quantile, and with per-domain evaluation domain_pcoc / domain_brier /
            domain_ece / domain_ece_quantile {d: value} and mean_pcoc / mean_brier / mean_ece / mean_ece_quantile, weighted like
            mean_auc; `calibration_table` returns the reliability tables.  Selection or early stopping by a calibration figure
            is not offered; intervals and the deltas of `compare` come with `calibration_ci`.
    recalibration: a `Recalibration` or a `PlattRecalibration` (from `fit_recalibration` on the validation loader, or the class's
            `fit`): every prediction goes through its map, clamped to [recalibration_eps, 1 - recalibration_eps] when that is positive, before anything is
            computed, so test(), calibration_table(), predict() and compare() report the recalibrated model under the same keys; raw
            against recalibrated on one checkpoint: Evaluator(model, ..).compare(Evaluator(model, .., recalibration=r), loader).  A map
            over more than one domain needs domain_idx.  Beta calibration, vector or matrix scaling, a "step" interpolation
            and selection by a calibration figure in `Runner` are not offered.
    precision: None, or "bf16" / "f32": the model is switched to it for the scoring pass and switched back afterwards, so two
            evaluators around ONE module can score it under two precisions (`compare`).
    calibration_ci: (needs calibration and bootstrap both set; ValueError otherwise) the clustered bootstrap over the calibration
            figures (`eval_calibration_bootstrap`: the evaluator's bins, replicate count, seed and level; clusters as `bootstrap`'s).
            test() adds, for fig in pcoc, brier, ece, ece_quantile, total_<fig>_boot_se/lo/hi and with per-domain evaluation
            domain_<fig>_boot_* {d: value} and mean_<fig>_boot_* (the mean formed per replicate); boot_valid covers them.  compare()
            adds total_<fig>_delta = figure(self) - figure(other) (two `eval_calibration` calls), total_<fig>_delta_boot_se/lo/hi from
            the per-replicate differences under shared weights, total_<fig>_z = delta / boot_se, and the domain_ and mean_ forms.
            ECE is biased upwards on small domains, so the interval of a delta deserves more trust than that of a level.  Without
            it every result dictionary and every launch is exactly as before.  Not offered: MCE replicates, per-bin reliability
            bands, BCa or studentised intervals, selection by a calibration figure in `Runner`."""

    def __init__(self, model, mode="multi", domain_idx=None, n_domain=1, domain_cnt_weight=None, is_evaluate_multi_domain=True,
                 user_idx=None, n_user=None, user_weight=None, auc_ci=False, precision=None, calibration=False, recalibration=None,
                 recalibration_eps=0.0, loss_ci=False, gauc_ci=False, bootstrap=None, bootstrap_seed=0, bootstrap_level=0.95,
                 calibration_ci=False, rank_at=None, rank_ci=False):
        self.model, self.mode = model, mode
        self.rank_at = None if rank_at is None else _rank_ks(rank_at)
        if self.rank_at is not None and user_idx is None:
            raise ValueError("rank_at needs user_idx, the column that holds a row's user: the top-K figures rank every user's own rows")
        self.rank_ci = bool(rank_ci)
        if self.rank_ci and self.rank_at is None:
            raise ValueError("rank_ci needs rank_at, the cut-offs of the top-K figures (and user_idx): it reports their standard errors")
        self.bootstrap = 0 if bootstrap is None else int(bootstrap)         # 0: off
        if bootstrap is not None and (isinstance(bootstrap, bool) or not 1 <= self.bootstrap <= BOOT_MAX_REP):
            raise ValueError(f"bootstrap must be None or a number of replicates in [1, {BOOT_MAX_REP}], not {bootstrap!r}")
        if not 0.0 < float(bootstrap_level) < 1.0:
            raise ValueError(f"bootstrap_level={bootstrap_level} must lie in (0, 1)")
        self.bootstrap_seed, self.bootstrap_level = int(bootstrap_seed), float(bootstrap_level)
        if recalibration is not None and recalibration.n_domain > 1 and domain_idx is None:
            raise ValueError(f"a recalibration map over {recalibration.n_domain} domains needs domain_idx, the column that holds a row's domain")
        if not 0.0 <= float(recalibration_eps) <= 0.5:
            raise ValueError(f"recalibration_eps={recalibration_eps} must lie in [0, 0.5]")
        self.recalibration, self.recalibration_eps = recalibration, float(recalibration_eps)
        self.auc_ci = bool(auc_ci)
        self.loss_ci, self.gauc_ci = bool(loss_ci), bool(gauc_ci)
        if self.gauc_ci and user_idx is None:
            raise ValueError("gauc_ci needs user_idx, the column that holds a row's user: the standard error is clustered by user")
        self.calibration_bins = 0 if calibration is False else (10 if calibration is True else int(calibration))   # 0: off
        if calibration is not False and not 1 <= self.calibration_bins <= MAX_CALIBRATION_BINS:
            raise ValueError(f"calibration must be a bool or a number of bins in [1, {MAX_CALIBRATION_BINS}], not {calibration!r}")
        self.calibration_ci = bool(calibration_ci)
        if self.calibration_ci and not (self.calibration_bins and self.bootstrap):
            raise ValueError("calibration_ci needs calibration (the bins) and bootstrap (the replicates) both set: its intervals are "
                             "the clustered bootstrap's over the calibration figures")
        if precision not in (None, "bf16", "f32"):
            raise ValueError(f"precision must be None, 'bf16' or 'f32', not {precision!r}")
        self.precision = precision
        self.domain_idx, self.n_domain = domain_idx, int(n_domain)
        self.domain_cnt_weight = domain_cnt_weight
        self.is_evaluate_multi_domain = bool(is_evaluate_multi_domain) and domain_idx is not None
        self.user_idx = user_idx
        if user_idx is not None:
            if n_user is None:
                raise ValueError("user_idx needs n_user, the size of the user id range")
            self.n_user = int(n_user)
            if isinstance(user_weight, dict):
                dense = torch.full((self.n_user,), math.nan, dtype=torch.float64)
                dense[torch.tensor(list(user_weight.keys()), dtype=torch.int64)] = torch.tensor(list(user_weight.values()), dtype=torch.float64)
                user_weight = dense
            self.user_weight = user_weight

    def predict(self, data_loader):
        """-> (pred f32 [n], label int16 [n], domain int32 [n] or None), all on the device."""
        return self._score(data_loader)[:3]

    def fit_recalibration(self, data_loader, method="isotonic", **kw):
        """One scoring pass over `data_loader` (the validation split) -> the map of every domain of the domain column (of all rows
        without one) fitted on the model's RAW predictions.  method "isotonic": a `Recalibration` (kw: `Recalibration.fit`'s
        min_rows, need_both_classes); "platt", "temperature", "bias": a `PlattRecalibration` (kw: `PlattRecalibration.fit`'s input,
        clip, gtol, max_iter, min_rows, need_both_classes, need_increasing)."""
        if method != "isotonic" and method not in PLATT_METHODS:
            raise ValueError(f"method={method!r} is none of {['isotonic'] + sorted(PLATT_METHODS)}")
        pred, label, domain, _ = self._score(data_loader, raw=True)
        n_domain = 1 if domain is None else self.n_domain
        if method == "isotonic":
            return Recalibration.fit(pred, label, domain, n_domain, **kw)
        return PlattRecalibration.fit(pred, label, domain, n_domain, method=method, **kw)

    def recommend(self, data_loader, k=10, item_idx=None, by="domain"):
        """The ranker's output: every user's k best-scored rows of `data_loader`, best first (`eval_topk`), from one scoring pass,
        recalibrated like `predict()`.  by "domain": lists per (domain, user) (needs domain_idx); by "user": lists per user over all
        rows.  item_idx: the column of X that holds the item id (>= 0) — a list then never repeats an item and equal scores order by
        item id; None: every row is its own candidate.  Returns the `TopK` with `label`, the entries' labels, attached (and `item`
        with item_idx); row indices count the rows in the order the loader yields them, as `predict()` returns them.  A NaN
        prediction or an id out of range raises ValueError, as in `test()`."""
        if self.user_idx is None:
            raise ValueError("recommend needs user_idx, the column that holds a row's user: a list ranks a user's own rows")
        if by not in ("domain", "user"):
            raise ValueError(f"by must be 'domain' or 'user', not {by!r}")
        if by == "domain" and self.domain_idx is None:
            raise ValueError("by='domain' needs domain_idx, the column that holds a row's domain; by='user' ranks over all rows")
        pred, label, domain, user, item = self._score(data_loader, with_item=True, item_idx=item_idx)
        per_domain = by == "domain"
        top = eval_topk(pred, user, self.n_user, domain if per_domain else None, self.n_domain if per_domain else 1, item, k)
        bad = int(top.err.item())
        if bad:
            raise ValueError(f"evaluation row {bad - 1}: NaN prediction, user outside [0, {self.n_user}), domain outside "
                             f"[0, {self.n_domain}) or negative item id")
        top.label = label[top.row.to(torch.int64)]
        return top

    def recommend_catalog(self, context, catalog, item_cols, k=10, seen=None, domain2group=None, tile_rows=32768, item_block=None):
        """Every context's k best items out of a catalogue: the user x item pool is written, scored and ranked tile by tile and never
        held as a whole.  context int32 [U, F]: one request per row, the model's full id row with the user side and the domain filled
        in; catalog int32 [I, C] with distinct, non-negative item ids in column 0 (ValueError otherwise: checked once, up front);
        item_cols: the C columns of X the catalogue's columns overwrite.  seen: None or `catalog_seen`'s pair — a context's seen items
        are left out.  Tiles hold Ub = max(1, tile_rows // Ib) contexts x Ib = min(I, item_block or tile_rows) items, so at most four
        batch sizes reach the model's plan cache; tile_rows = 32768 was the fastest of 4096, 8192, 16384 and 32768 in
        tools/catalog_bench.py's run (profiles/catalog_bench.txt).  Per tile: `catalog_rows`, the eval-mode forward as `predict()` runs it — mode
        "multi": model(X).gather(1, group) with group = domain2group[X[:, domain_idx]] (domain2group is required there, and
        domain_idx); "cdc": model(X, mode='split'), which gathers by the model's own table; "single": model(X) — the evaluator's
        recalibration with the tile's domain column, `catalog_topk`.  One read at the end, of the error words: a NaN score, a negative
        id or a domain outside domain2group raises ValueError naming the context.  Returns the `CatalogTopK`; one list per context,
        contexts are never grouped by user."""
        k = _catalog_k(k)
        if self.mode == "multi" and (domain2group is None or self.domain_idx is None):
            raise ValueError("mode 'multi' needs domain2group, the tower group of every domain, and domain_idx, the column that holds a "
                             "row's domain: the pool's rows are scored by their domain's tower")
        if isinstance(tile_rows, bool) or int(tile_rows) != tile_rows or not 1 <= tile_rows < 1 << 31:
            raise ValueError(f"tile_rows={tile_rows!r} is no integer in [1, 2^31)")
        if item_block is not None and (int(item_block) != item_block or item_block < 1):
            raise ValueError(f"item_block={item_block!r} is no positive integer")
        catalog, _ = _id_matrix(torch.as_tensor(catalog), "catalog")
        context, _ = _id_matrix(torch.as_tensor(context), "context")
        ids = catalog[:, 0]
        if int(ids.min()) < 0:                                              # the up-front reads
            raise ValueError("the catalogue holds a negative item id (column 0)")
        if torch.unique(ids).numel() != ids.numel():
            raise ValueError("the catalogue repeats an item id (column 0): ids must be distinct")
        _need_device("recommend_catalog", context)
        dev = context.device
        catalog = catalog.to(dev)
        (U, _), I = context.shape, catalog.shape[0]
        ib = min(I, int(item_block or tile_rows))
        ub = min(U, max(1, int(tile_rows) // ib))
        g_of_d = None if self.mode != "multi" else _flat(torch.as_tensor(domain2group), torch.int64, dev)
        recal = self.recalibration
        need_domain = g_of_d is not None or (recal is not None and recal.n_domain > 1)
        state = CatalogTopK.empty(U, k, dev)
        rows_err = torch.zeros(1, dtype=torch.int32, device=dev)
        model = self.model
        was_training = model.training
        model.eval()
        was_precision = None
        if self.precision is not None:
            was_precision = getattr(model, "base_model_instance", model).precision
            model.set_precision(self.precision)
        try:
            with torch.no_grad():
                for u0 in range(0, U, ub):
                    nu = min(ub, U - u0)
                    for i0 in range(0, I, ib):
                        ni = min(ib, I - i0)
                        X, group, domain = catalog_rows(context, catalog, item_cols, u0, nu, i0, ni, g_of_d,
                                                        self.domain_idx if need_domain else None, err=rows_err)
                        if self.mode == "cdc":
                            pred = model(X, mode='split')
                        elif self.mode == "multi":
                            pred = model(X).gather(1, group.reshape(-1, 1))
                        else:
                            pred = model(X)
                        pred = pred.reshape(-1).to(torch.float32)
                        if recal is not None:
                            pred = recal.apply(pred, domain if recal.n_domain > 1 else None, self.recalibration_eps)
                        catalog_topk(state, pred, catalog, u0, nu, i0, ni, seen)
        finally:
            model.train(was_training)
            if was_precision is not None and was_precision != self.precision:
                model.set_precision(was_precision)
        bad_domain, bad = torch.cat([rows_err, state.err]).cpu().tolist()  # the one read
        if bad_domain:
            raise ValueError(f"context {bad_domain - 1}: domain outside domain2group's [0, {g_of_d.numel()})")
        if bad:
            raise ValueError(f"context {bad - 1}: NaN prediction or negative item id among its candidates")
        return state

    def _score(self, data_loader, raw=False, with_item=False, item_idx=None):
        """predict() and the user column: -> (pred, label, domain or None, user int32 [n] or None); with a recalibration map (and not
        raw) pred has gone through it.  with_item (recommend): a fifth entry follows, X[:, item_idx] int32 [n], None without item_idx"""
        model = self.model
        was_training = model.training
        model.eval()
        was_precision = None
        if self.precision is not None:
            was_precision = getattr(model, "base_model_instance", model).precision
            model.set_precision(self.precision)
        preds, labels, domains, users, items = [], [], [], [], []
        try:
            with torch.no_grad():
                for batch in (self._domain_batches(*data_loader) if self.mode == "cdc" else data_loader):
                    if self.mode == "cdc":
                        d, X, y = batch
                        pred = model(X, mode='split', domain_i=d)
                    elif self.mode == "multi":
                        X, y, group = batch
                        pred = model(X).gather(1, group.reshape(-1, 1).to(torch.int64))
                    else:
                        X, y = batch
                        pred = model(X)
                    preds.append(pred.reshape(-1).to(torch.float32))
                    labels.append(y.reshape(-1).to(torch.int16))
                    if self.domain_idx is not None:
                        domains.append(X[:, self.domain_idx].to(torch.int32))
                    if self.user_idx is not None:
                        users.append(X[:, self.user_idx].to(torch.int32))
                    if item_idx is not None:
                        items.append(X[:, item_idx].to(torch.int32))
        finally:
            model.train(was_training)
            if was_precision is not None and was_precision != self.precision:
                model.set_precision(was_precision)
        if not preds:
            raise ValueError("empty evaluation set")
        pred, domain = torch.cat(preds), (torch.cat(domains) if domains else None)
        if self.recalibration is not None and not raw:
            pred = self.recalibration.apply(pred, domain if self.recalibration.n_domain > 1 else None, self.recalibration_eps)
        out = pred, torch.cat(labels), domain, (torch.cat(users) if users else None)
        return out + (torch.cat(items) if items else None,) if with_item else out

    @staticmethod
    def _domain_batches(loaders, domain_batch_seq):
        """Run.get_domain_data in 'valid' / 'test' mode (run.py:507-526): a generator per domain, restarted when exhausted; the
        sequence holds ceil(rows_d / bs) entries of d, so one pass visits every row of every domain once."""
        gens = {}
        for d in domain_batch_seq:
            d = int(d)
            if d not in gens:
                gens[d] = iter(loaders[d])
            try:
                X, y = next(gens[d])
            except StopIteration:
                gens[d] = iter(loaders[d])
                X, y = next(gens[d])
            yield d, X, y

    def test(self, data_loader):
        """The reference's result_dict: total_auc, total_loss (+ domain_auc, domain_loss, mean_auc, mean_loss); with user_idx also
        total_gauc (+ domain_gauc, mean_gauc); with auc_ci also total_auc_se (+ domain_auc_se, mean_auc_se); with calibration also
        total_pcoc, total_brier, total_ece, total_ece_quantile (+ domain_* and mean_* of the four); with loss_ci also total_loss_se
        (+ domain_loss_se, mean_loss_se); with gauc_ci also total_gauc_se (+ domain_gauc_se; no mean_gauc_se: the per-domain GAUCs
        share users and are not independent); with bootstrap also total_*_boot_se/lo/hi, domain_*_boot_*, mean_*_boot_* for auc, loss
        and (with user_idx) gauc, and boot_valid; with calibration_ci the same *_boot_* keys for pcoc, brier, ece and ece_quantile;
        with rank_at also total_<fig>@<K> (+ domain_<fig>@<K>, mean_<fig>@<K>) for ndcg, recall, precision, hit, mrr and
        total_rank_users (+ domain_rank_users); with rank_ci also total_<fig>@<K>_se (+ domain_<fig>@<K>_se) and, with bootstrap,
        the total_/domain_/mean_<fig>@<K>_boot_* keys."""
        pred, label, domain, user = self._score(data_loader)
        multi = self.is_evaluate_multi_domain
        auc, loss, rows, pos = eval_metrics(pred, label, domain if multi else None, self.n_domain if multi else 1)
        if user is not None:                                   # queued behind the metrics: still nothing has been read back
            gauc = eval_gauc(pred, label, user, self.n_user, domain if multi else None, self.n_domain if multi else 1, self.user_weight)[0]
        if self.rank_ci:                                       # likewise queued: eval_rank's figures bit for bit, variances, replicates
            rank = eval_rank_ci(pred, label, user, self.n_user, domain if multi else None, self.n_domain if multi else 1, self.rank_at,
                                self.user_weight, n_rep=self.bootstrap, seed=self.bootstrap_seed)
        elif self.rank_at is not None:                         # likewise queued
            rank = eval_rank(pred, label, user, self.n_user, domain if multi else None, self.n_domain if multi else 1, self.rank_at,
                             self.user_weight)
        if self.auc_ci:                                        # likewise queued
            ci_var = eval_auc_ci(pred, label, domain if multi else None, self.n_domain if multi else 1).var
        if self.calibration_bins:                              # likewise queued
            cal = eval_calibration(pred, label, domain if multi else None, self.n_domain if multi else 1, self.calibration_bins)
        if self.loss_ci:                                       # likewise queued
            loss_var = eval_loss_ci(pred, label, domain if multi else None, self.n_domain if multi else 1).var
        if self.gauc_ci:                                       # likewise queued
            gauc_var = eval_gauc_ci(pred, label, user, self.n_user, domain if multi else None, self.n_domain if multi else 1,
                                    self.user_weight).var
        if self.bootstrap:                                     # likewise queued, summaries included
            boot = self._bootstrap(pred, label, domain, user, multi)
            stats = {"auc": boot.auc, "loss": boot.loss}
            if user is not None:
                stats["gauc"] = boot.gauc
            if self.calibration_ci:                            # likewise queued: the same weights over the calibration figures
                cb = self._calibration_bootstrap(pred, label, domain, user, multi)
                stats.update({"pcoc": cb.pcoc, "brier": cb.brier, "ece": cb.ece, "ece_quantile": cb.ece_q})
            if self.rank_ci:
                stats.update(self._rank_stats(rank.reps))
            boot_sum = self._boot_summary(stats, rows, multi)
        auc, loss, rows, pos = auc.cpu().tolist(), loss.cpu().tolist(), rows.cpu().tolist(), pos.cpu().tolist()   # the one sync
        bad = int(eval_metrics.last_err.item())
        if bad:
            raise ValueError(f"evaluation row {bad - 1}: NaN prediction, label outside {{0,1}} or domain outside [0, {self.n_domain})")
        if pos[-1] == 0 or pos[-1] == rows[-1]:
            raise ValueError("Only one class present in y_true. ROC AUC score is not defined in that case.")   # run.py:685
        result = {"total_auc": auc[-1], "total_loss": loss[-1]}
        if multi:
            domain_auc, domain_loss = {}, {}
            mean_auc, mean_loss = 0, 0
            for d in range(self.n_domain):
                if rows[d] == 0:
                    continue                                   # pandas groupby yields no group for an absent domain
                domain_auc[d], domain_loss[d] = auc[d], loss[d]
                w = self._weight(d)
                mean_auc += w * auc[d]
                mean_loss += w * loss[d]
            result.update({"domain_auc": domain_auc, "domain_loss": domain_loss, "mean_auc": mean_auc, "mean_loss": mean_loss})
        if user is not None:
            gauc = gauc.cpu().tolist()
            bad = int(eval_gauc.last_err.item())
            if bad:
                raise ValueError(f"evaluation row {bad - 1}: user outside [0, {self.n_user})")
            result["total_gauc"] = gauc[-1]
            if multi:
                domain_gauc = {d: gauc[d] for d in range(self.n_domain) if rows[d] > 0}
                result["domain_gauc"] = domain_gauc
                result["mean_gauc"] = sum(self._weight(d) * v for d, v in domain_gauc.items())     # as mean_auc; NaN when a domain has no countable user
        if self.rank_at is not None:                           # a bad user id has been raised above: the two calls flag the same rows
            figures, counted = torch.stack(rank[:len(RANK_FIGURES)]).cpu().tolist(), rank.counted.cpu().tolist()
            present = [d for d in range(self.n_domain) if rows[d] > 0] if multi else []
            for fig, per_k in zip(RANK_FIGURES, figures):
                for K, v in zip(self.rank_at, per_k):
                    result[f"total_{fig}@{K}"] = v[-1]
                    if multi:
                        result[f"domain_{fig}@{K}"] = {d: v[d] for d in present}
                        result[f"mean_{fig}@{K}"] = sum(self._weight(d) * v[d] for d in present)   # as mean_gauc: NaN when a domain counts no user
            result["total_rank_users"] = counted[-1]
            if multi:
                result["domain_rank_users"] = {d: counted[d] for d in present}
        if self.rank_ci:
            for fig, per_k in zip(RANK_FIGURES, rank.var.cpu().tolist()):
                for K, v in zip(self.rank_at, per_k):
                    result[f"total_{fig}@{K}_se"] = _se(v[-1])
                    if multi:
                        result[f"domain_{fig}@{K}_se"] = {d: _se(v[d]) for d in present}
        if self.auc_ci:
            var = ci_var.cpu().tolist()
            result["total_auc_se"] = _se(var[-1])
            if multi:
                present = [d for d in range(self.n_domain) if rows[d] > 0]
                result["domain_auc_se"] = {d: _se(var[d]) for d in present}
                result["mean_auc_se"] = _se(sum(self._weight(d) ** 2 * var[d] for d in present))   # NaN when a summed domain's variance is
        if self.calibration_bins:
            figures = {"pcoc": cal.pcoc, "brier": cal.brier, "ece": cal.ece, "ece_quantile": cal.ece_q}
            figures = {k: v.cpu().tolist() for k, v in figures.items()}
            bad = int(eval_calibration.last_err.item())
            if bad:
                raise ValueError(f"evaluation row {bad - 1}: prediction outside [0, 1]")
            for k, v in figures.items():
                result["total_" + k] = v[-1]
                if multi:
                    result["domain_" + k] = {d: v[d] for d in range(self.n_domain) if rows[d] > 0}
                    result["mean_" + k] = sum(self._weight(d) * x for d, x in result["domain_" + k].items())     # as mean_auc
        if self.loss_ci:
            var = loss_var.cpu().tolist()
            bad = int(eval_loss_ci.last_err.item())
            if bad:
                raise ValueError(f"evaluation row {bad - 1}: prediction outside [0, 1]")
            result["total_loss_se"] = _se(var[-1])
            if multi:
                present = [d for d in range(self.n_domain) if rows[d] > 0]
                result["domain_loss_se"] = {d: _se(var[d]) for d in present}
                result["mean_loss_se"] = _se(sum(self._weight(d) ** 2 * var[d] for d in present))  # as mean_auc_se: disjoint row sets
        if self.gauc_ci:
            var = gauc_var.cpu().tolist()
            result["total_gauc_se"] = _se(var[-1])
            if multi:
                result["domain_gauc_se"] = {d: _se(var[d]) for d in range(self.n_domain) if rows[d] > 0}
        if self.bootstrap:
            self._boot_report(result, list(stats), boot_sum, rows, multi)
        return result

    def _bootstrap(self, pred, label, domain, user, multi, pred_b=None, gauc=None):
        """the replicates of one evaluation set: clusters are the users when user_idx is set, otherwise rows"""
        return eval_bootstrap(pred, label, user, self.n_user if user is not None else None, domain if multi else None,
                              self.n_domain if multi else 1, self.bootstrap, self.bootstrap_seed,
                              self.user_weight if user is not None else None, gauc=gauc, pred_b=pred_b)

    def _rank_stats(self, reps, suffix=""):
        """replicates [n_rep, 5, len(rank_at), seg] -> {"<fig>@<K><suffix>": [n_rep, seg]} in `_boot_summary`'s form"""
        return {f"{fig}@{K}{suffix}": reps[:, f, k] for f, fig in enumerate(RANK_FIGURES) for k, K in enumerate(self.rank_at)}

    def _calibration_bootstrap(self, pred, label, domain, user, multi, pred_b=None):
        """the calibration figures' replicates under `_bootstrap`'s clusters, replicate count and seed, over the evaluator's bins"""
        return eval_calibration_bootstrap(pred, label, user, self.n_user if user is not None else None, domain if multi else None,
                                          self.n_domain if multi else 1, self.calibration_bins, self.bootstrap, self.bootstrap_seed,
                                          pred_b=pred_b)

    def _boot_summary(self, stats, rows, multi):
        """stats {name: replicates [n_rep, seg]}, rows: eval's row counts [seg] (device) -> [len(stats), 4, seg + 1] f64 on the device:
        (se, lo, hi, valid) of every column and, last, of the mean over the present domains, formed PER REPLICATE with mean_auc's
        weights (a replicate in which a present domain is NaN gives a NaN mean and is left out).  Nothing is read back."""
        out = []
        for reps in stats.values():
            if multi:
                w = torch.tensor([self._weight(d) for d in range(self.n_domain)], dtype=torch.float64, device=reps.device)
                present = rows[:self.n_domain] > 0
                mean = torch.where(present, reps[:, :self.n_domain] * w, torch.zeros((), dtype=torch.float64, device=reps.device)).sum(1)
            else:
                mean = torch.full((reps.shape[0],), math.nan, dtype=torch.float64, device=reps.device)
            se, lo, hi, valid = summarize_bootstrap(torch.cat([reps, mean[:, None]], 1), self.bootstrap_level)
            out.append(torch.stack([se, lo, hi, valid.to(torch.float64)]))
        return torch.stack(out)

    def _boot_report(self, result, names, boot_sum, rows, multi):
        """total_<name>_boot_se / _lo / _hi, with per-domain evaluation domain_<name>_boot_* {d: value} over the present domains and
        mean_<name>_boot_*; boot_valid = the smallest number of valid replicates over everything reported (the mean's only when
        domain_cnt_weight is set: without it every mean is NaN).  -> {name: [se, lo, hi, valid] host lists over the columns (the
        domains, ALL rows, the mean)}"""
        summ = boot_sum.cpu().tolist()
        bad = int(eval_bootstrap.last_err.item())
        if bad:
            raise ValueError(f"evaluation row {bad - 1}: NaN prediction, label outside {{0,1}}, domain outside [0, {self.n_domain}) or "
                             f"user outside range")
        if self.calibration_ci:
            bad = int(eval_calibration_bootstrap.last_err.item())
            if bad:
                raise ValueError(f"evaluation row {bad - 1}: prediction outside [0, 1]")
        n_all = len(summ[0][0]) - 2                            # columns: the domains, ALL rows, the mean
        present = [d for d in range(self.n_domain) if rows[d] > 0] if multi else []
        valid = []
        for name, s in zip(names, summ):
            for k, what in enumerate(("se", "lo", "hi")):
                result[f"total_{name}_boot_{what}"] = s[k][n_all]
                if multi:
                    result[f"domain_{name}_boot_{what}"] = {d: s[k][d] for d in present}
                    result[f"mean_{name}_boot_{what}"] = s[k][n_all + 1]
            valid += [s[3][n_all]] + [s[3][d] for d in present]
            if multi and self.domain_cnt_weight is not None:
                valid.append(s[3][n_all + 1])
        result["boot_valid"] = int(min(valid))
        return dict(zip(names, summ))

    def calibration_table(self, data_loader):
        """One scoring pass -> (table, table_q, segments): the equal-width and the equal-mass reliability table as
        `CalibrationTable`s of host numpy arrays [len(segments), n_bins] (count, positives, mean_pred, pos_rate, pred_min, pred_max;
        NaN in an empty bin), and `segments`, the row order: the domain ids 0..n_domain-1 with per-domain evaluation, then "all".
        The bins are those of `calibration` (10 when it is off)."""
        pred, label, domain, _ = self._score(data_loader)
        multi = self.is_evaluate_multi_domain
        cal = eval_calibration(pred, label, domain if multi else None, self.n_domain if multi else 1, self.calibration_bins or 10)
        first = 0 if multi else 1                              # without per-domain evaluation the one domain IS "all"
        table, table_q = (CalibrationTable(*(f[first:].cpu().numpy() for f in t)) for t in (cal.table, cal.table_q))
        bad = int(eval_calibration.last_err.item())
        if bad:
            raise ValueError(f"evaluation row {bad - 1}: NaN prediction or prediction outside [0, 1], label outside {{0,1}} or domain "
                             f"outside [0, {self.n_domain})")
        return table, table_q, (list(range(self.n_domain)) if multi else []) + ["all"]

    def compare(self, other, data_loader):
        """Paired comparison of this evaluator's model with `other`'s (an Evaluator) on ONE evaluation set: the loader is scored
        with self.model, then with other.model — `other` may wrap the same module under another `precision`; the passes run one
        after the other.  Both passes must see the same labels and domain columns in the same order (ValueError otherwise: a
        shuffling loader shows here).  Returns total_delta = AUC(self) - AUC(other), total_delta_se (DeLong's paired standard
        error) and total_z = delta / se, and with per-domain evaluation domain_delta / domain_delta_se / domain_z {d: value} and
        mean_delta / mean_delta_se / mean_z, weighted by domain_cnt_weight like mean_auc.  z is NaN for 0 / 0 (identical
        predictions) and +-inf for a non-zero delta with se 0.  With loss_ci set on this evaluator the same nine keys for the log-loss
        (total_loss_delta, total_loss_delta_se, total_loss_z, domain_loss_*, mean_loss_*: raw against recalibrated shows here, where
        the AUC delta is 0); with gauc_ci set total_gauc_delta, total_gauc_delta_se, total_gauc_z and domain_gauc_* (no mean_gauc_*,
        as in test()) — then both passes must also see the same user column.  With bootstrap set total_delta_boot_se/lo/hi (+ domain_
        and mean_ forms), the *_loss_delta_boot_* forms with loss_ci and the *_gauc_delta_boot_* forms with gauc_ci
        (mean_gauc_delta_boot_* included), and boot_valid: the replicates weight both models' rows alike; with user_idx the users are
        resampled and both passes must see the same user column.  With calibration_ci, for fig in pcoc, brier, ece, ece_quantile:
        total_<fig>_delta (figure(self) - figure(other), from two `eval_calibration` calls), total_<fig>_delta_boot_se/lo/hi,
        total_<fig>_z = delta / boot_se by the rules above, and the domain_ and mean_ forms.  With rank_ci, for fig in ndcg, recall,
        precision, hit, mrr and every K of rank_at: total_<fig>@<K>_delta, _delta_se and _z (+ the domain_ forms) from one paired
        `eval_rank_ci` call, and with bootstrap the *_delta_boot_* forms, mean_<fig>@<K>_delta and mean_<fig>@<K>_z = delta / boot_se;
        both passes must then see the same user column."""
        pred_a, label, domain, user = self._score(data_loader)
        pred_b, label_b, domain_b, user_b = other._score(data_loader)
        if label.shape != label_b.shape or not torch.equal(label, label_b):
            raise ValueError("the two scoring passes saw different labels: compare() needs a loader that yields the same rows in the same order")
        if (domain is None) != (domain_b is None) or (domain is not None and not torch.equal(domain, domain_b)):
            raise ValueError("the two scoring passes saw different domain columns: compare() needs a loader that yields the same rows in the same order")
        if (self.gauc_ci or self.rank_ci) and (user_b is None or not torch.equal(user, user_b)):
            raise ValueError("the two scoring passes saw different user columns: compare() with gauc_ci or rank_ci needs the same user_idx in both "
                             "evaluators and a loader that yields the same rows in the same order")
        if self.bootstrap and user is not None and (user_b is None or not torch.equal(user, user_b)):
            raise ValueError("the two scoring passes saw different user columns: compare() with bootstrap resamples users and needs the "
                             "same user_idx in both evaluators and a loader that yields the same rows in the same order")
        multi = self.is_evaluate_multi_domain
        ci = eval_auc_ci(pred_a, label, domain if multi else None, self.n_domain if multi else 1, pred_b=pred_b)
        if self.loss_ci:                                       # queued behind the AUC's: still nothing has been read back
            lci = eval_loss_ci(pred_a, label, domain if multi else None, self.n_domain if multi else 1, pred_b=pred_b)
        if self.gauc_ci:                                       # likewise queued
            gci = eval_gauc_ci(pred_a, label, user, self.n_user, domain if multi else None, self.n_domain if multi else 1,
                               self.user_weight, pred_b=pred_b)
        if self.rank_ci:                                       # likewise queued: the replicates of both vectors come with it
            rci = eval_rank_ci(pred_a, label, user, self.n_user, domain if multi else None, self.n_domain if multi else 1, self.rank_at,
                               self.user_weight, pred_b=pred_b, n_rep=self.bootstrap, seed=self.bootstrap_seed)
        if self.bootstrap:                                     # likewise queued: per-replicate differences under shared weights
            boot = self._bootstrap(pred_a, label, domain, user, multi, pred_b=pred_b, gauc=self.gauc_ci)
            stats = {"delta": boot.auc - boot.auc_b}
            if self.loss_ci:
                stats["loss_delta"] = boot.loss - boot.loss_b
            if self.gauc_ci:
                stats["gauc_delta"] = boot.gauc - boot.gauc_b
            if self.calibration_ci:                            # likewise queued: both point figures and the shared-weight replicates
                cal_a = eval_calibration(pred_a, label, domain if multi else None, self.n_domain if multi else 1, self.calibration_bins)
                cal_err_a = eval_calibration.last_err
                cal_b = eval_calibration(pred_b, label, domain if multi else None, self.n_domain if multi else 1, self.calibration_bins)
                cb = self._calibration_bootstrap(pred_a, label, domain, user, multi, pred_b=pred_b)
                cal_delta = {"pcoc": cal_a.pcoc - cal_b.pcoc, "brier": cal_a.brier - cal_b.brier, "ece": cal_a.ece - cal_b.ece,
                             "ece_quantile": cal_a.ece_q - cal_b.ece_q}
                stats.update({"pcoc_delta": cb.pcoc - cb.pcoc_b, "brier_delta": cb.brier - cb.brier_b, "ece_delta": cb.ece - cb.ece_b,
                              "ece_quantile_delta": cb.ece_q - cb.ece_q_b})
            if self.rank_ci:
                stats.update(self._rank_stats(rci.reps - rci.reps_b, "_delta"))
            boot_sum = self._boot_summary(stats, ci.rows, multi)
        delta, var, rows = ci.delta.cpu().tolist(), ci.var_delta.cpu().tolist(), ci.rows.cpu().tolist()
        bad = int(eval_auc_ci.last_err.item())
        if bad:
            raise ValueError(f"evaluation row {bad - 1}: NaN prediction, label outside {{0,1}} or domain outside [0, {self.n_domain})")
        se = _se(var[-1])
        result = {"total_delta": delta[-1], "total_delta_se": se, "total_z": _z(delta[-1], se)}
        if multi:
            present = [d for d in range(self.n_domain) if rows[d] > 0]
            d_se = {d: _se(var[d]) for d in present}
            mean_delta = sum(self._weight(d) * delta[d] for d in present)
            mean_se = _se(sum(self._weight(d) ** 2 * var[d] for d in present))
            result.update({"domain_delta": {d: delta[d] for d in present}, "domain_delta_se": d_se,
                           "domain_z": {d: _z(delta[d], d_se[d]) for d in present},
                           "mean_delta": mean_delta, "mean_delta_se": mean_se, "mean_z": _z(mean_delta, mean_se)})
        if self.loss_ci:
            delta, var = lci.delta.cpu().tolist(), lci.var_delta.cpu().tolist()
            bad = int(eval_loss_ci.last_err.item())
            if bad:
                raise ValueError(f"evaluation row {bad - 1}: prediction outside [0, 1]")
            se = _se(var[-1])
            result.update({"total_loss_delta": delta[-1], "total_loss_delta_se": se, "total_loss_z": _z(delta[-1], se)})
            if multi:
                d_se = {d: _se(var[d]) for d in present}
                mean_delta = sum(self._weight(d) * delta[d] for d in present)
                mean_se = _se(sum(self._weight(d) ** 2 * var[d] for d in present))
                result.update({"domain_loss_delta": {d: delta[d] for d in present}, "domain_loss_delta_se": d_se,
                               "domain_loss_z": {d: _z(delta[d], d_se[d]) for d in present},
                               "mean_loss_delta": mean_delta, "mean_loss_delta_se": mean_se, "mean_loss_z": _z(mean_delta, mean_se)})
        if self.gauc_ci:
            delta, var = gci.delta.cpu().tolist(), gci.var_delta.cpu().tolist()
            bad = int(eval_gauc_ci.last_err.item())
            if bad:
                raise ValueError(f"evaluation row {bad - 1}: user outside [0, {self.n_user})")
            se = _se(var[-1])
            result.update({"total_gauc_delta": delta[-1], "total_gauc_delta_se": se, "total_gauc_z": _z(delta[-1], se)})
            if multi:
                d_se = {d: _se(var[d]) for d in present}
                result.update({"domain_gauc_delta": {d: delta[d] for d in present}, "domain_gauc_delta_se": d_se,
                               "domain_gauc_z": {d: _z(delta[d], d_se[d]) for d in present}})
        if self.bootstrap:
            summ = self._boot_report(result, list(stats), boot_sum, rows, multi)
        if self.calibration_ci:
            bad = max(int(cal_err_a.item()), int(eval_calibration.last_err.item()))
            if bad:
                raise ValueError(f"evaluation row {bad - 1}: prediction outside [0, 1]")
            n_all = self.n_domain if multi else 1              # the "all rows" column; the mean's follows it
            for k, v in cal_delta.items():
                delta, se = v.cpu().tolist(), summ[k + "_delta"][0]
                result[f"total_{k}_delta"] = delta[-1]
                result[f"total_{k}_z"] = _z(delta[-1], se[n_all])
                if multi:
                    mean_delta = sum(self._weight(d) * delta[d] for d in present)
                    result.update({f"domain_{k}_delta": {d: delta[d] for d in present},
                                   f"domain_{k}_z": {d: _z(delta[d], se[d]) for d in present},
                                   f"mean_{k}_delta": mean_delta, f"mean_{k}_z": _z(mean_delta, se[n_all + 1])})
        if self.rank_ci:
            deltas, variances = rci.delta.cpu().tolist(), rci.var_delta.cpu().tolist()
            bad = int(eval_rank_ci.last_err.item())
            if bad:
                raise ValueError(f"evaluation row {bad - 1}: user outside [0, {self.n_user})")
            n_all = self.n_domain if multi else 1              # the "all rows" column; the mean's follows it
            for fig, d_k, v_k in zip(RANK_FIGURES, deltas, variances):
                for K, delta, var in zip(self.rank_at, d_k, v_k):
                    k, se = f"{fig}@{K}", _se(var[-1])
                    result.update({f"total_{k}_delta": delta[-1], f"total_{k}_delta_se": se, f"total_{k}_z": _z(delta[-1], se)})
                    if multi:
                        d_se = {d: _se(var[d]) for d in present}
                        result.update({f"domain_{k}_delta": {d: delta[d] for d in present}, f"domain_{k}_delta_se": d_se,
                                       f"domain_{k}_z": {d: _z(delta[d], d_se[d]) for d in present}})
                        if self.bootstrap:                     # the mean's error exists only over the replicates
                            mean_delta = sum(self._weight(d) * delta[d] for d in present)
                            result.update({f"mean_{k}_delta": mean_delta,
                                           f"mean_{k}_z": _z(mean_delta, summ[k + "_delta"][0][n_all + 1])})
        return result

    def _weight(self, d):
        w = self.domain_cnt_weight
        if w is None:
            return math.nan
        return float(w[d])
