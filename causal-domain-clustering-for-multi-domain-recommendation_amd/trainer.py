"""Step driver of the HIP path: one training step with the reference's order of operations
(Run.train, run.py:470-497):

    pred = model(X) ; loss = BCE(pred.gather(1, group), y) ; loss += model.get_regularization_loss()
    model.zero_grad() ; loss.backward() ; optimizer.step() ; loss.item()

Here the whole step is a fixed sequence of launches (plan forward -> BCE+grad -> plan backward -> table and
dense Adam with the L2 term folded in), replayable as ONE hipGraph.  Nothing synchronises with the host:
`TrainStep.step()` returns device scalars; read them (loss.item()) only when you log.
"""
import ctypes as C
import os

import torch

from . import _lib as L
from .optim import FusedAdam


def _run_steps(steps):
    """a launch piece of a data-parallel sequence: plan steps issued on the current stream"""
    def fn():
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        for s_ in steps:
            s_(st)
    return fn


def _merge_pieces(seq):
    """[(is_comm, fn)] -> [(is_comm, [fn...])]: neighbouring launch pieces fused into one segment"""
    merged = []
    for is_comm, fn in seq:
        if merged and not is_comm and not merged[-1][0]:
            merged[-1][1].append(fn)
        else:
            merged.append((is_comm, [fn]))
    return merged


class LossWeights:
    """How a TrainStep weights the rows of its loss — torch's `F.binary_cross_entropy(p, y, weight=w, reduction='mean')` with
           w[b] = (row[b] * domain_weight[X[b, domain_idx]]) * (pos_weight if y[b] > 0 else 1)
    formed on the device once per step, in fp32 and in this order (csrc/rowops.hip cdc_stage_weights).
      row            True: every step(...) call is given `weight=` (fp32 [B] or [B,1] on the device)
      domain_weight  one weight per id of field `domain_idx` (a sequence or tensor of feature_dims[domain_idx] floats); an id outside
                     the table weighs 0 (check_ids() reports such ids)
      pos_weight     the weight of the positive rows (the hard-label case of BCEWithLogitsLoss(pos_weight=))
    The mean stays over the batch's rows (1 / global batch), NOT over sum(w): normalise the weights for a weighted mean.  Weights
    are finite and expected to be >= 0; they are not validated on the device."""

    def __init__(self, row=False, domain_weight=None, domain_idx=None, pos_weight=1.0):
        self.row = bool(row)
        self.pos_weight = float(pos_weight)
        if not (self.pos_weight == self.pos_weight and abs(self.pos_weight) != float("inf")):
            raise ValueError("pos_weight must be finite")
        if (domain_weight is None) != (domain_idx is None):
            raise ValueError("domain_weight and domain_idx belong together")
        self.domain_idx = None if domain_idx is None else int(domain_idx)
        if domain_weight is not None:
            dw = torch.as_tensor(domain_weight).detach().to(device="cpu", dtype=torch.float32).reshape(-1).clone()
            if dw.numel() == 0 or not bool(torch.isfinite(dw).all()):
                raise ValueError("domain_weight must hold at least one weight, all finite")
            if self.domain_idx < 0:
                raise ValueError("domain_idx must be a field index")
            domain_weight = dw
        self.domain_weight = domain_weight

    @property
    def active(self):
        return self.row or self.domain_weight is not None or self.pos_weight != 1.0

    def check(self, feature_dims):
        """against the model the step is built for: one weight per id of the domain field"""
        if self.domain_weight is None:
            return
        if self.domain_idx >= len(feature_dims):
            raise ValueError(f"domain_idx {self.domain_idx} is not one of the model's {len(feature_dims)} fields")
        if self.domain_weight.numel() != int(feature_dims[self.domain_idx]):
            raise ValueError(f"domain_weight holds {self.domain_weight.numel()} weights, field {self.domain_idx} has "
                             f"{int(feature_dims[self.domain_idx])} ids")


class TrainStep:
    """mode:
         "multi"   multi-tower models (PLE / MMoE / CDC split): pred = model(X).gather(1, group)  (run.py:481-484)
         "single"  DCN / DCNv2: pred = model(X)                                                   (run.py:486-488)
         "mean"    CDC warm-up: pred = mean over the towers of model(X)                           (cdc.py:100-102, run.py:616)
         "single_group"  one output column, but the model itself reads the row's group (HiNet: model(X, group))  (run.py:476-479)
         "star"    STAR: pred, y = model(X, group, targets=y) — rows partitioned by domain, every   (run.py:476-479,
                   partition through its own tower, loss on the group-ordered targets              star.py:109-181)
       train_mode=False: the step runs with the module in EVAL mode (BatchNorm on its running statistics, no dropout) but
       still back-propagates and updates — what the reference's CDC loop does after its first evaluation pass, which
       leaves the model in eval() (run.py:550-551 sets it, nothing sets it back before the training that follows)."""

    def __init__(self, model, optimizer: FusedAdam, batch_size, mode="multi", use_graph=False, dist=None, sync_bn=True,
                 table_dist=None, shard_slack=1.5, train_mode=True, overlap=True, overlap_waves=2, sort_ahead=True, fuse_gather=False,
                 defer_dw_reduce=None, global_rows=None, cap_rows=None, tower_one_launch=True, rows_dense_one_launch=True,
                 loss_weights=None, bwd_tail_one_launch=True):
        """sync_bn (data parallel only): BatchNorm statistics over the GLOBAL batch, as the reference's single process
        computes them — two small all-reduces per BatchNorm launch; False = per-rank statistics.
        table_dist (data parallel only): "sharded" (row r owned by rank r % world; default with the lazy table optimiser)
        or "replicated" (every rank applies the global batch's table update).  shard_slack: capacity of the per-owner,
        per-field row lists as a multiple of the even share B/world (an overflow raises in check_ids()).
        global_rows / cap_rows (data parallel, the ragged last global batch of an epoch: TrainStep.sibling): the batch's true global
        size (the BCE mean runs over it; this rank's share is batch_size) and the largest share any rank holds (row-list capacities
        are a property of the exchange, equal on every rank).
        overlap / overlap_waves / sort_ahead / fuse_gather (single GPU, lazy table; for tests and A/B runs — the defaults are what is
        measured and shipped): the replay slice in the background on a second chain (waves per SIMD of its capped grid), the next
        batch's row sort on that chain (step(..., next_X=); sort_ahead=False ignores next_X), the catch-up launch that also writes
        the gathered embeddings (slower: profiles/round3/README.md section 3).
        loss_weights: a LossWeights — per-row, per-domain and positive-class weights of the loss, decided here so that a captured
        graph has fixed pointers; None (or one that weights nothing) is the unweighted step.
        bwd_tail_one_launch (single GPU): the embeddings' grad-input launch and the batched grad-weight launch that end the backward
        go out as one launch (cdc_glinear_bwd_xw) where the plan's tail has that form (Plan.bwd_tail; bwd_tail_fused tells);
        bit-identical results."""
        self.model, self.opt, self.B, self.mode = model, optimizer, int(batch_size), mode
        self.lib = L.load()
        self.dist = dist
        self.sync_bn = bool(sync_bn)
        self.world = 1 if dist is None else dist.world_size
        self.dp_on = self.world > 1 or bool(getattr(dist, "force", False))     # force: the collective path with one rank
        self.global_B = self.B * self.world if global_rows is None else int(global_rows)
        self._shard_slack = float(shard_slack)
        dev = optimizer.device
        self.device = dev
        self.train_mode = bool(train_mode)
        self._overlap_ok, self._overlap_waves = bool(overlap), int(overlap_waves)
        # the two updates that end a single-GPU step with the lazy table (the step's rows; the dense parameters) as one launch
        self._rows_dense_one = bool(rows_dense_one_launch) and not self.dp_on
        self.tower_one_launch = bool(tower_one_launch)        # the fused towers' forward and backward as one launch (cdc_tower_step)
        self.bwd_tail_one_launch = bool(bwd_tail_one_launch)  # the backward's last grad-input launch rides the grad-weight launch
        self._per_launch_timing = False                       # profile(overlap=False) is running: every launch of bwd_steps on its own
        # split-K slabs of the batched grad-weight launches summed by the dense Adam launch (single GPU; under data parallelism the
        # reduced gradient is what is all-reduced)
        self._defer_dw = (not self.dp_on) if defer_dw_reduce is None else (bool(defer_dw_reduce) and not self.dp_on)
        assert mode in ("multi", "single", "mean", "star", "single_group")
        # the plan shares the optimiser's step counter (dropout stream) and its flat gradient arena
        self.holder = self._build_plan()
        self.plan = self.holder.plan
        self.emb = self.holder.emb_op
        self.out = self.holder.outputs[0]
        self.y = torch.zeros(self.B, dtype=torch.int16, device=dev)
        self.group = torch.zeros(self.B, dtype=torch.int64, device=dev) if mode == "multi" else None
        if mode == "single_group":
            self.group_in = self.holder.inputs[1]                 # int64 [B] read by the plan's group-selection launch
        if mode == "star":
            self.group = self.holder.inputs[1]                    # the partition kernel reads the domain of every row here
            self.order = self.holder.extra_outputs[0]             # row order after the partition (ascending group)
            self.y_perm = torch.zeros(self.B, dtype=torch.int16, device=dev)
        self.loss = torch.zeros(1, dtype=torch.float32, device=dev)
        # loss weights: the step's effective row weights in a static buffer the (replayed) weighted BCE launch reads; written by
        # one eager launch beside the staging launch of every step()
        if loss_weights is not None and not isinstance(loss_weights, LossWeights):
            raise TypeError("loss_weights must be a LossWeights")
        self.loss_weights = loss_weights if (loss_weights is not None and loss_weights.active) else None
        self.w = None
        if self.loss_weights is not None:
            self.loss_weights.check(model.feature_dims)
            self.w = torch.ones(self.B, dtype=torch.float32, device=dev)
            dw = self.loss_weights.domain_weight
            self._domain_w = None if dw is None else dw.to(dev)
            if mode == "star":
                self.w_perm = torch.ones(self.B, dtype=torch.float32, device=dev)
        # ids are checked against their FIELD's vocabulary while a batch is staged (an id past it that still lies inside the table
        # aliases another field's row: check_ids reports it)
        self.field_dims_dev = torch.tensor([int(d) for d in model.feature_dims], dtype=torch.int32, device=dev)
        self.alias = torch.zeros(1, dtype=torch.int32, device=dev)
        # the step's sum(l2*w^2), formed inside the launch sequence; lazy table: the optimiser's accumulator itself (see _reg)
        self.reg = self.opt.reg_sum[0] if self.opt.table_mode == "lazy" else torch.zeros((), dtype=torch.float64, device=dev)
        self.use_graph = use_graph
        self.graph = None
        self._stage_graphs = {}
        self._step_graphs = {}            # data parallel over RCCL: the whole step (launches + collectives) as one graph per sequence
        self._one_graph_ok = None
        self._dp_seq = None
        self._warm = 0
        self._reg_checked = False
        if table_dist is None:
            table_dist = "sharded" if optimizer.table_mode == "lazy" else "replicated"
        assert table_dist in ("sharded", "replicated")
        self.table_dist = table_dist if self.dp_on else "replicated"
        if self.dp_on and self.table_dist == "replicated":
            F, D = self.emb.F, self.emb.D
            self.idx_all = torch.empty((self.global_B, F), dtype=torch.int32, device=dev)
            self.dE_all = torch.empty((self.global_B, F * D), dtype=torch.float32, device=dev)
            self._loss_behind_arena()
        if self.dp_on and self.table_dist == "sharded":
            if optimizer.table_mode != "lazy":
                raise ValueError("the row-sharded table needs table_mode='lazy'")
            F, D, N = self.emb.F, self.emb.D, self.world
            Bc = self.B if cap_rows is None else int(cap_rows)           # the largest local batch of the step over the ranks
            assert Bc >= self.B
            cap = min(Bc, int(-(-Bc // N) * float(shard_slack)) + 16)
            if N * cap > L.SORT_MAX_ROWS:
                raise ValueError(f"world {N} x list capacity {cap} exceeds the per-field sort limit {L.SORT_MAX_ROWS}")
            self.cap, self.Bv = cap, N * cap                          # Bv: rows of the owner-side batch
            z = dict(device=dev)
            self.send_ids = torch.full((N, cap, F), -1, dtype=torch.int32, **z)
            self.recv_ids = torch.full((N, cap, F), -1, dtype=torch.int32, **z)
            self.recv_ids_alt = torch.full((N, cap, F), -1, dtype=torch.int32, **z)   # the id exchange one step ahead lands here
            self.slot_of = torch.zeros((F, self.B), dtype=torch.int32, **z)
            self.overflow = torch.zeros(1, dtype=torch.int32, **z)
            self.rows_send = torch.zeros((N, cap, F * D), dtype=torch.float32, **z)
            self.rows_recv = torch.zeros((N, cap, F * D), dtype=torch.float32, **z)
            self.grads_send = torch.zeros((N, cap, F * D), dtype=torch.float32, **z)
            self.grads_recv = torch.zeros((N, cap, F * D), dtype=torch.float32, **z)
            self.zero_offsets = torch.zeros(F, dtype=torch.int32, **z)
            optimizer.own_mod, optimizer.own_rem = N, dist.rank
            self._loss_behind_arena()
        # ---- how a step goes out, decided once -------------------------------------------------------------------------
        lazy_one = optimizer.table_mode == "lazy" and not self.dp_on
        D = self.emb.D
        # single GPU, lazy table: the catch-up launch writes the gathered embeddings itself (csrc/embedding.hip
        # k_lazy_catchup_gather); needs a row's 16-byte lanes inside one wave.  Off by default: measured at C2
        # (profiles/round2/README.md) the fused launch takes 48 us against 28.5 + 7.2 us for catch-up + gather — the wave that owns the
        # domain column's three rows writes ~B positions on its own while the rest of the chip has finished; it wins only where no
        # row is looked up by more than a few samples
        self._fuse_gather_ok = lazy_one and bool(fuse_gather) and D % 4 == 0 and 64 % (D // 4) == 0
        # single GPU, lazy table, slice in the background: the sort + dedupe of batch t+1's rows (30 us of three dependent launches
        # that read nothing but the ids) goes out on the side chain of step t, behind the slice, when the caller names the next batch
        # (step(..., next_X=)); step t+1 then starts at the catch-up.  Otherwise every step sorts its own batch at the head of the
        # side chain
        self._ahead_ok = lazy_one and self._overlap_ok and bool(sort_ahead) and not self._fuse_gather_ok
        # data parallel, row-sharded table: the local sort, the bucketing and the id exchange of batch t+1 leave step t+1's critical
        # path when the caller names the next batch; see _dp_sequence_sharded.  (A forced one-rank group has no transfer for the
        # moved work to hide under — measured 0.803 -> 0.818 ms/step on the one-GPU box, the step there is bound by the host-side
        # issue of its segments — so it takes part only with sort_ahead="force", which the RCCL call-path test sets)
        self._ahead_dp_ok = (self.dp_on and self.table_dist == "sharded" and bool(sort_ahead) and
                             (self.world > 1 or sort_ahead == "force"))
        # the staging launch also begins the step (cdc_stage_batch_next: ++step, accumulators cleared) where the step's first
        # launch is not one that can: one GPU with the lazy table (the sort may have run a step ahead), the data-parallel look-ahead
        self._stage_begins = lazy_one or self._ahead_dp_ok
        self._parity, self._sorted_for = 0, None          # the look-ahead's bookkeeping (_lookahead)
        self._graphs, self._dp_seqs = {}, {}              # per (have, prefetch, p): single GPU graphs, data-parallel sequences
        if self._ahead_ok or self._ahead_dp_ok:
            self.ids_next = torch.zeros_like(self.emb.ids)

    def _loss_behind_arena(self):
        """Data parallel: the loss scalar sits right behind the used part of the flat gradient arena, so ONE all-reduce covers the
        dense gradients and the loss."""
        used = max(self.plan._arena_used, 1)
        assert self.opt.grad_arena.numel() > used
        self.arena_and_loss = self.opt.grad_arena[:used + 1]
        self.loss = self.opt.grad_arena[used:used + 1]

    def _build_plan(self):
        model, opt = self.model, self.opt
        B = self.B
        dev = opt.device
        from .functional import PlanHolder
        from . import plan as P

        def build():
            plan = P.Plan(dev, B, precision=model.precision, training=self.train_mode,
                          dropout=float(getattr(model, "dropout_p", 0.0)) if self.train_mode else 0.0,
                          seed=int(getattr(model, "seed", 0)), step_dev=opt.step_dev, grad_arena=opt.grad_arena,
                          dist=self.dist if self.sync_bn else None, defer_dw_reduce=self._defer_dw)
            emb = model.embedding.describe(plan)
            outs, ins, extra = model.describe(plan, emb, grouped=True) if self.mode == "star" else model.describe(plan, emb)
            plan.finalize(outs)
            return PlanHolder(plan, [emb.ids] + ins, outs, emb_op=emb, extra_outputs=extra)

        was = model.training
        model.train(self.train_mode)                 # the ops read module.training while describing themselves
        try:
            return model._cache().get(model, ("train_step", id(opt), self.train_mode, self.mode == "star",
                                               bool(self.sync_bn and self.dp_on), bool(self.dp_on), self._defer_dw), B, build)
        finally:
            model.train(was)

    # ------------------------------------------------------------------------------------------
    def _find_head(self):
        """The launch that turns the tower logits into the predictions the loss reads: a single sigmoid row-dot launch whose
        groups are the columns of `self.out`, in order.  Its backward can form the BCE gradient itself (cdc_rowdot_bwd's fused
        BCE): one launch and a round trip through d_out less per step.  Returns that launch's argument block or None."""
        from . import plan as P
        out = self.out
        for op in self.plan.ops:
            if isinstance(op, (P.TowerHead, P.TowerChain)) and op.sigmoid and op.out.key == out.key:
                if len(op.bwd_args) == 1 and op.M == self.B:
                    self._head_op = op
                    return op.bwd_args[0]
                return None
        for op in self.plan.ops:
            if not isinstance(op, P.RowDot) or not op.sigmoid or op.row_offsets is not None or len(op.groups) != out.cols:
                continue
            if all(g["out"].key == out.slice(i, i + 1).key for i, g in enumerate(op.groups)):
                return op.bwd_args[0] if len(op.bwd_args) == 1 and op.M == self.B else None
        return None

    def _head_lookup(self):
        head = self.__dict__.get("_head", False)
        if head is False:
            self._head_op = None
            head = self._head = self._find_head()
            self._fuse_bce = head is not None and self.mode in ("multi", "single", "single_group")
            if self._fuse_bce:
                self._bce_partial = torch.zeros(L.MAX_GROUPS * L.ROWDOT_PARTS, dtype=torch.float64, device=self.device)
            from . import plan as P
            # the towers' two launches as one (csrc/tower.hip cdc_tower_step): the fused loss, one GPU
            self._tower_both = (self._head_op if self._fuse_bce and self.tower_one_launch and not self.dp_on and
                                isinstance(self._head_op, P.TowerChain) and self.plan.dist is None else None)
        return head

    def _towers_one_launch(self, on):
        """around the launches of a step (the plan, and with it the op, may be shared with a trainer that wants the other form)"""
        self._head_lookup()
        if self._tower_both is not None:
            self._tower_both.one_launch = bool(on)

    @property
    def bwd_tail_fused(self):
        """Does the single-GPU launch sequence (_launch) end its backward with cdc_glinear_bwd_xw instead of two launches?"""
        return self.bwd_tail_one_launch and not self.dp_on and self.plan.bwd_tail is not None

    def _backward(self, st):
        """plan.backward(), with the fused tail where it is in use: bwd_steps up to the last grad-input launch, then one launch for
        it and the grad-weight launch behind it.  Per-launch timing on one stream (profile(overlap=False)) keeps the two launches:
        their names and durations are what the per-kernel tables are built from."""
        plan = self.plan
        if not (self.bwd_tail_fused and not self._per_launch_timing):
            for fn in plan.bwd_steps:
                fn(st)
            return
        x_step, w_step, fused = plan.bwd_tail
        for fn in plan.bwd_steps:
            if fn is x_step:
                fused(st)
            elif fn is not w_step:
                fn(st)

    def _bce(self):
        og = self.out.grad
        head = self._head_lookup()
        if head is not None:
            # the argument block belongs to the (cached, possibly shared) plan: set for this trainer before every backward
            if self._fuse_bce:
                head.bce_group = None if self.group is None else self.group.data_ptr()
                head.bce_y_i16, head.bce_y_f32 = self.y.data_ptr(), None
                head.bce_loss = self.loss.data_ptr()
                if hasattr(type(head), "bce_partial"):            # (the fused tower launch keeps its partial sums in its own workspace)
                    head.bce_partial = self._bce_partial.data_ptr()
                head.bce_inv_count = 1.0 / self.global_B
                # loss weights ride the same launch; cleared for an unweighted step that shares the plan with a weighted one
                head.bce_weight = None if self.w is None else self.w.data_ptr()
                return
            head.bce_y_i16 = head.bce_y_f32 = head.bce_weight = None
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        if self.w is not None:
            if self.mode == "mean":
                L.launch("cdc_bce_mean_weighted_fwd_bwd", self.lib.cdc_bce_mean_weighted_fwd_bwd,
                         (self.out.ptr, self.out.ld, self.y.data_ptr(), None, self.w.data_ptr(), self.loss.data_ptr(), og.ptr, og.ld,
                          self.B, self.out.cols, 1.0 / self.global_B), st)
                return
            y, group, w = self.y, self.group, self.w
            if self.mode == "star":                               # targets[order] (star.py:181) and their weights, one column
                order = self.order.long()
                torch.index_select(self.y, 0, order, out=self.y_perm)
                torch.index_select(self.w, 0, order, out=self.w_perm)
                y, group, w = self.y_perm, None, self.w_perm
            L.launch("cdc_bce_weighted_fwd_bwd", self.lib.cdc_bce_weighted_fwd_bwd,
                     (self.out.ptr, self.out.ld, None if group is None else group.data_ptr(), y.data_ptr(), None, w.data_ptr(),
                      self.loss.data_ptr(), og.ptr, og.ld, self.B, self.out.cols, 1.0 / self.global_B), st)
            return
        if self.mode == "mean":
            L.launch("cdc_bce_mean_fwd_bwd", self.lib.cdc_bce_mean_fwd_bwd,
                     (self.out.ptr, self.out.ld, self.y.data_ptr(), None, self.loss.data_ptr(), og.ptr, og.ld, self.B, self.out.cols,
                      1.0 / self.global_B), C.c_void_p(torch.cuda.current_stream().cuda_stream))
            return
        y, group = self.y, self.group
        if self.mode == "star":                                   # targets[order] (star.py:181), one column
            torch.index_select(self.y, 0, self.order.long(), out=self.y_perm)
            y, group = self.y_perm, None
        L.launch("cdc_bce_fwd_bwd", self.lib.cdc_bce_fwd_bwd,
                 (self.out.ptr, self.out.ld, None if group is None else group.data_ptr(), y.data_ptr(), None,
                  self.loss.data_ptr(), og.ptr, og.ld, self.B, self.out.cols, 1.0 / self.global_B),
                 C.c_void_p(torch.cuda.current_stream().cuda_stream))

    def _reg(self):
        # part of the (graph-replayed) launch sequence, so that step() issues nothing else per call.  Dense table mode: the
        # streaming pass sums w^2 of the whole table every step (reg_sum[1]).  Lazy table: nobody walks the table in a step;
        # the table's term is the value of the last refresh_table_reg() (flush + exact sum), see there; the first dense Adam launch
        # of the step adds it to the dense parameters' sum, so `reg` IS the optimiser's accumulator and no launch is issued here.
        if self.opt.table_mode != "lazy":
            torch.add(self.opt.reg_sum[0], self.opt.reg_sum[1], alpha=self.opt.l2_table, out=self.reg)

    def refresh_table_reg(self):
        """Lazy table: brings every row to the current step and re-evaluates the table's share of the reference's reported loss
        (run.py:489: `loss += get_regularization_loss()`, i.e. l2 * sum(w^2) over the WHOLE table, model/layer.py:31,96-112).  The
        value is exact for the weights the NEXT step's forward sees, and is what `step()` adds to its reg figure until the next
        refresh (per step it changes by ~lr * 2 * l2 * sum|w|: 2e-8 relative at the reference's settings).  One pass over
        the table: called when the step is built, at the start of an epoch and where the reference's value is looked at (the
        logging steps of train_epoch / CDCTrainer), not every step.  Row-sharded table: every rank sums the rows it owns and the
        figures are added up across ranks (a collective: call it on every rank)."""
        sharded = self.dp_on and self.table_dist == "sharded"
        return self.opt.refresh_table_reg(self.dist if sharded else None)

    def _launch(self, have, prefetch, p):
        """Single GPU: the whole step as one launch sequence (one hipGraph per (have, prefetch, p) when use_graph).  Lazy table:
        have = this batch's sorted rows are in workspace a<p> (sorted by the previous step), prefetch = sort the batch in ids_next
        into workspace a<1-p>; begin_step's work was done by the staging launch (cdc_stage_batch_next).
            side:  [sort] catch-up * | slice, [sort of the next batch]
            main:  weight shadows    | (wait *) gather, forward, BCE, backward, grad-weight launches, dense Adam | join | row update
        The backward ends with the embeddings' grad-input launch and the batched grad-weight launch; where the plan's tail has that form
        (Plan.bwd_tail) and bwd_tail_one_launch is set, the two go out as ONE launch (cdc_glinear_bwd_xw, _backward):
            ... cgc_mid_bwd, level-1 grad-input, [embedding grad-input + grad-weight tiles] | join | rows + dense Adam
        The side chain is a second stream on its own hardware queue (two branches of the hipGraph when captured) when the slice runs
        in the BACKGROUND (overlap, the default), and the main stream itself otherwise: no fork, no event, no join, and the slice
        goes out with its full grid.  The fork sits at the head of the step: the weight-shadow launch reads nothing of the table and
        covers the cross-queue edge (by the kernel trace, profiles/round3/step_timeline.txt, the fork-after-catch-up form left 12 us
        between the catch-up and the first forward launch).
        The slice is VALU-only and touches no row of the batch (those are at step t-1 after the catch-up and are skipped); in the
        background it goes out capped (overlap_waves per SIMD) at the lowest issue priority (cdc_embed_lazy_flush_bg) while the
        chain's kernels raise theirs (CDC_PRIO_MAIN): it takes the issue cycles the chain leaves idle while waiting on L2 / LDS / MFMA
        results.  Measured at C2 (profiles/round3/README.md): serial 0.550 ms/step; side by side with the full grid 0.596 (round 2:
        its 4096 workgroups take every wave slot); capped at two waves per SIMD, lowest priority, table update behind a single join:
        0.515.  The table update needs the slice finished: it goes last on the main chain, behind the one join.
        fuse_gather: the catch-up launch also writes the gathered embeddings (+ shadow; hot rows staged in LDS and written by a whole
        workgroup), and the plan's own gather launch is skipped."""
        opt, plan, emb = self.opt, self.plan, self.emb
        B, F, D = self.B, emb.F, emb.D
        main = torch.cuda.current_stream()
        st = C.c_void_p(main.cuda_stream)
        self._towers_one_launch(True)
        try:
            if opt.table_mode != "lazy":
                opt.begin_step()
                plan.forward()
                self._bce()
                self._backward(st)
                opt.table_step(emb.idx, emb.out.grad.root, B, F, D)
                opt.dense_step(plan.param_grads, plan._param_refs, plan.grad_slabs)
                self._reg()
                return
            cur, nxt = f"a{p}", f"a{1 - p}"
            bg, fused = self._overlap_ok, self._fuse_gather_ok
            side = self._side_stream() if bg else main
            # measured (same box, ms/step): fork after the catch-up + row update behind the join 0.411 / 0.412; catch-up on the side
            # chain under the weight-shadow launch 0.403; row update on the side chain as well (waiting for dE by an event, beside the
            # grad-weight launches and the dense Adam) 0.420 / 0.424 — two more cross-queue edges cost more than the 24 us they free;
            # main chain captured FIRST behind the catch-up (so that it stays on the origin queue and the side chain takes the
            # cross-queue edge): the replayed graph then starts the slice 150 us late, 0.476
            if bg:
                side.wait_stream(main)
            with torch.cuda.stream(side):
                if not have:
                    opt.begin_step_sort(emb.ids, emb.offsets, B, F, D, tag=cur, err=emb.err if fused else None, begin=False)
                if fused:
                    oh, ldh = plan.shadow_view(emb.out) if (plan.use_g2 and plan.has_shadow(emb.out)) else (None, 0)
                    opt.catchup_gather(B, F, D, cur, emb.out.ptr, oh, ldh)
                else:
                    opt.catchup(B, F, D, cur)
                if bg:
                    rows_ready = torch.cuda.Event()
                    rows_ready.record(side)
                opt.flush_slice(background_waves=self._overlap_waves if bg else 0)
                if prefetch:      # behind the slice (ahead of it the sort delays the whole side chain into the backward: 0.401 -> 0.443 ms;
                                  # held back by an event until the backward chain has run: 0.408 -> 0.427)
                    opt.begin_step_sort(self.ids_next, emb.offsets, B, F, D, tag=nxt, begin=False)
            nws = plan.n_wshadow_steps
            for fn in plan.fwd_steps[:nws]:
                fn(st)
            if bg:
                main.wait_event(rows_ready)
            for fn in plan.fwd_steps[nws:]:
                if not (fused and fn is emb.fwd_step):
                    fn(st)
            self._bce()
            self._backward(st)                # (ends with the grad-weight launches: plan.deferred_dw_steps, or the fused tail)
            if self._rows_dense_one:
                # the step's rows and the dense parameters in one launch behind the join (optim.rows_and_dense_step)
                if bg:
                    main.wait_stream(side)
                opt.rows_and_dense_step(emb.idx, emb.out.grad.root, B, F, D, plan.param_grads, plan._param_refs, plan.grad_slabs, tag=cur)
            else:
                opt.dense_step(plan.param_grads, plan._param_refs, plan.grad_slabs)
                # (the row update on the side chain beside these two, or on this chain in front of them as soon as the slice has ended,
                # was measured again in round 4: 0.345 and 0.350 ms against 0.338 — every additional cross-queue edge of the replayed
                # graph moves nodes to another hardware queue and costs ~10 us where it lands, profiles/round4/README.md section 6)
                if bg:
                    main.wait_stream(side)
                opt.table_step(emb.idx, emb.out.grad.root, B, F, D, tag=cur)
            self._reg()
        finally:
            self._towers_one_launch(False)

    def _lookahead(self, X, nx):
        """(have, prefetch, p) of a step with the look-ahead sort, and the bookkeeping moved on: have = X is the batch the previous
        step announced (its rows were sorted into buffer p), prefetch = this step sorts nx into buffer 1 - p.  The remembered tensor
        is kept alive (its storage cannot be handed to another batch) and its version pins its contents."""
        key = (X.data_ptr(), X._version) if torch.is_tensor(X) else None
        have = self._sorted_for is not None and self._sorted_for[:2] == key
        p = self._parity
        if nx is not None:
            self._parity = 1 - p
            self._sorted_for = (nx.data_ptr(), nx._version, nx)
        else:
            self._sorted_for = None
        return have, nx is not None, p

    def _drop_graphs(self):
        """releases every captured graph (before the process group is destroyed: DataParallel.close)"""
        self._step_graphs.clear()
        self._stage_graphs.clear()
        self._graphs.clear()
        self.graph = None

    def _side_stream(self):
        if getattr(self, "_side", None) is None:
            self._side = torch.cuda.Stream(device=self.device)
        return self._side

    # ---- data parallel: launch segments separated by the collectives (each segment replayable as a graph) ---------------
    def _dp_sequence(self):
        """[(is_comm, fn)]: dense gradients: ONE sum all-reduce of the flat arena (the loss already carries
        1/global_batch); table: every rank applies the identical update from the all-gathered (row index, row gradient)
        pairs of the global batch; BatchNorm: statistics all-reduced inside the plan (sync_bn)."""
        opt, plan, emb, dp = self.opt, self.plan, self.emb, self.dist
        F, D = emb.F, emb.D

        def stage0():
            opt.begin_step()
            opt.table_index(emb.ids, emb.offsets, emb.idx, self.B, F)

        def catchup():
            if opt.table_mode == "lazy":
                opt.sort_rows(self.idx_all, self.global_B, F, D)
                opt.catchup(self.global_B, F, D)
                opt.flush_slice()

        def exchange():
            dp.all_reduce_sum(self.arena_and_loss)                      # dense gradients + the loss scalar behind them
            dp.all_gather_rows(self.dE_all, emb.out.grad.root)

        def update():
            opt.table_step(self.idx_all, self.dE_all, self.global_B, F, D)
            opt.dense_step(plan.param_grads, plan._param_refs, plan.grad_slabs)
            self._reg()

        seq = [(False, stage0), (True, lambda: dp.all_gather_rows(self.idx_all, emb.idx)), (False, catchup)]
        seq += [(is_comm, _run_steps(steps)) for is_comm, steps in plan.segments(plan.fwd_steps)]
        seq.append((False, self._bce))
        seq += [(is_comm, _run_steps(steps)) for is_comm, steps in plan.segments(plan.bwd_steps)]
        seq += [(True, exchange), (False, update)]
        return _merge_pieces(seq)

    def _dp_sequence_sharded(self, ahead=False, have=False, prefetch=False, p=0):
        """Row-sharded table: [(is_comm, [fn...])].  Per step and rank the table work is that of the LOCAL batch:
            sort local rows -> bucket by owner | a2a ids | owner: merge the sorted lists, catch-up, gather |
            a2a rows | expand, forward, BCE, backward, per-row gradient sums, pack | all-reduce arena, a2a grads |
            owner: per-row sums over the senders, Adam update of its rows; dense Adam.
        ahead (step(..., next_X=) in use): the step counter is advanced by the staging launch, and the first two items — which
        read nothing but ids — run one step AHEAD: with `prefetch` the NEXT batch (ids_next) is sorted and bucketed in the segment
        of the grad-weight launches (the local sort workspace and the slot lists are free once `pack` has run) and its id exchange
        is started behind the gradient all-reduce, into the OTHER of two receive buffers (this step's owner update still reads
        its own); with `have` this step starts at the owner's `serve`, after awaiting that exchange.  p: which receive buffer
        holds THIS step's lists."""
        opt, plan, emb, dp = self.opt, self.plan, self.emb, self.dist
        B, F, D, N, cap, Bv = self.B, emb.F, emb.D, self.world, self.cap, self.Bv
        lib = self.lib
        bufs = (self.recv_ids, self.recv_ids_alt)
        recv_cur, recv_nxt = bufs[p], bufs[1 - p]
        # round 4: with the whole step in ONE graph (or issued eagerly) a second chain can run beside the dense one, as on one GPU:
        # the owner's replay slice (capped, lowest priority) from the catch-up to the row update, and the next batch's sort and
        # bucketing beside the grad-weight launches.  Launch SEGMENTS cannot hold a fork in one and its join in another: there
        # (gloo rehearsal with graphs, or after a refused capture) everything stays on the one chain
        side_ok = self._overlap_ok and (not self.use_graph or (getattr(dp, "capturable", False) and self._one_graph_ok is not False))

        def st():
            return C.c_void_p(torch.cuda.current_stream().cuda_stream)

        def sort_bucket(ids, begin):
            ws = opt.begin_step_sort(ids, emb.offsets, B, F, D, "local", err=emb.err, begin=begin)   # [++step,] index, sort
            L.launch("cdc_shard_bucket", lib.cdc_shard_bucket,
                     (ws["uniq"].data_ptr(), ws["cnt"].data_ptr(), self.send_ids.data_ptr(), self.slot_of.data_ptr(),
                      self.overflow.data_ptr(), B, F, N, cap), st())

        def stage0():
            sort_bucket(emb.ids, begin=not ahead)

        def stage0_next():
            sort_bucket(self.ids_next, begin=False)

        def serve():
            opt.sort_rows(recv_cur, Bv, F, D, "owner", runs=N)           # each sender's list is sorted
            opt.catchup(Bv, F, D, "owner")
            if side_ok:                               # the slice of the owned rows in the background, until the row update
                main, side = torch.cuda.current_stream(), self._side_stream()
                side.wait_stream(main)
                with torch.cuda.stream(side):
                    opt.flush_slice(background_waves=self._overlap_waves)
            L.launch("cdc_embed_gather_fwd(owner)", lib.cdc_embed_gather_fwd,
                     (recv_cur.data_ptr(), self.zero_offsets.data_ptr(), opt.table.data_ptr(), self.rows_send.data_ptr(),
                      None, None, Bv, F, D, opt.table.shape[0]), st())

        emb_shadow = plan.shadow_convert_step(emb.out) if (plan.use_g2 and plan.has_shadow(emb.out)) else None

        def expand():
            ws = opt._workspace(B, F, D, "local")
            L.launch("cdc_shard_expand", lib.cdc_shard_expand,
                     (self.rows_recv.data_ptr(), ws["uniq"].data_ptr(), ws["cnt"].data_ptr(), ws["seg"].data_ptr(),
                      ws["perm"].data_ptr(), self.slot_of.data_ptr(), emb.out.ptr, B, F, D, N, cap), st())
            if emb_shadow is not None:                    # the gather launch this replaces also wrote the embeddings' bf16 shadow
                emb_shadow(st())

        def pack():
            ws = opt._workspace(B, F, D, "local")
            opt._segment_sum(ws, emb.out.grad.root, B, F, D, st())
            L.launch("cdc_shard_pack", lib.cdc_shard_pack,
                     (ws["rowgrad"].data_ptr(), ws["uniq"].data_ptr(), ws["cnt"].data_ptr(), self.slot_of.data_ptr(),
                      self.grads_send.data_ptr(), B, F, D, N, cap), st())

        pending = {}

        def exchange_rows_start():
            # the row gradients travel while the grad-weight launches (which nothing here depends on) run
            pending["grads"] = dp.all_to_all_start(self.grads_recv, self.grads_send)

        def exchange_finish():
            dp.wait(pending.pop("grads", None))
            dp.all_reduce_sum(self.arena_and_loss)                      # dense gradients + the loss scalar behind them
            if prefetch:                                                # the next step's row lists travel under this step's updates
                self._ids_pending = dp.all_to_all_start(recv_nxt, self.send_ids)

        def ids_await():
            dp.wait(self.__dict__.pop("_ids_pending", None))

        def update():
            if side_ok:
                torch.cuda.current_stream().wait_stream(self._side_stream())      # the slice (and the look-ahead sort) are done
            if side_ok:
                # the owner's row update and the dense parameters in one launch, as on one GPU (optim.rows_and_dense_step)
                opt.rows_and_dense_step(recv_cur, self.grads_recv, Bv, F, D, plan.param_grads, plan._param_refs, plan.grad_slabs, tag="owner",
                                        short_segments=True)
                self._reg()
                return
            opt.table_step(recv_cur, self.grads_recv, Bv, F, D, "owner", short_segments=True)
            opt.flush_slice()                           # off the rows-exchange critical path: after the owner's update
            opt.dense_step(plan.param_grads, plan._param_refs, plan.grad_slabs)
            self._reg()

        def stage0_next_side():
            # the next batch's sort + bucketing beside the grad-weight launches (its workspaces are free once `pack` has run)
            main, side = torch.cuda.current_stream(), self._side_stream()
            side.wait_stream(main)
            with torch.cuda.stream(side):
                sort_bucket(self.ids_next, begin=False)

        def join_side():
            torch.cuda.current_stream().wait_stream(self._side_stream())

        if have:
            seq = [(True, ids_await), (False, serve)]
        else:
            seq = [(False, stage0), (True, lambda: dp.all_to_all(recv_cur, self.send_ids)), (False, serve)]
        seq += [(True, lambda: dp.all_to_all(self.rows_recv, self.rows_send)), (False, expand)]
        fwd = [s_ for s_ in plan.fwd_steps if s_ is not emb.fwd_step]
        seq += [(is_comm, _run_steps(steps)) for is_comm, steps in plan.segments(fwd)]
        seq.append((False, self._bce))
        late = set(id(s_) for s_ in plan.deferred_dw_steps)
        seq += [(is_comm, _run_steps(steps)) for is_comm, steps in plan.segments([s_ for s_ in plan.bwd_steps if id(s_) not in late])]
        if prefetch and side_ok:
            seq += [(False, pack), (False, stage0_next_side), (True, exchange_rows_start), (False, _run_steps(plan.deferred_dw_steps)),
                    (False, join_side)]
        else:
            seq += [(False, pack), (True, exchange_rows_start), (False, _run_steps(plan.deferred_dw_steps))]
            if prefetch:
                seq.append((False, stage0_next))
        seq += [(True, exchange_finish), (False, update)]
        return _merge_pieces(seq)

    def gather_table(self):
        """Row-sharded table: bring every owner's rows up to date and give every rank the whole table (and its Adam
        moments) — before state_dict(), evaluation, or a switch to another trainer.  Host-synchronising collectives."""
        opt = self.opt
        opt.flush_table()
        if not self.dp_on or self.table_dist != "sharded":
            return
        R = opt.table.shape[0]
        own = (torch.arange(R, device=self.device) % self.world == self.dist.rank).to(torch.float32).unsqueeze(1)
        for t in (opt.table.data, opt.table_m, opt.table_v):
            t.mul_(own)                                   # x + 0 + ... + 0 is exact: the all-reduce is a row broadcast
            self.dist.all_reduce_sum(t)
        opt.table_last.fill_(int(opt.step_dev.item()))

    def _step_dp(self, X=None, nx=None):
        key = None
        if self._ahead_dp_ok:
            key = self._lookahead(X, nx)
            if not key[0]:
                self.__dict__.pop("_ids_pending", None)                 # (an exchange started for a batch that did not come: its
                                                                        #  buffer is simply overwritten by the next one)

        def sequence():
            if key is not None:
                seq = self._dp_seqs.get(key)
                if seq is None:
                    seq = self._dp_seqs[key] = self._dp_sequence_sharded(ahead=True, have=key[0], prefetch=key[1], p=key[2])
                return seq
            if self._dp_seq is None:
                self._dp_seq = self._dp_sequence_sharded() if self.table_dist == "sharded" else self._dp_sequence()
            return self._dp_seq

        seq = sequence()
        if self.use_graph and self._warm >= 2 and self._one_graph_ok is not False and getattr(self.dist, "capturable", False):
            # ONE graph for the whole step, collectives included (round 4: RCCL collectives capture and replay on this stack; what hung
            # in rounds 2-3 was destroy_process_group() with such a graph alive — DataParallel.close() releases them first).  The
            # five-segment cut (launch segments replayed, collectives issued by the host in between) is the fallback
            g = self._step_graphs.get(key)
            if g is None:
                # capture from a quiescent state: an exchange the previous (eager) step left in flight is awaited OUTSIDE the capture
                # (inside, ids_await then finds nothing: a replayed predecessor has joined its own exchange at its end), the device is
                # drained, and the RCCL watchdog thread gets time to retire the eager collectives it is still polling — it must not
                # query events while this thread captures (seen once in a full-suite run: the capture ended "unjoined" and the
                # watchdog then died on an event "last recorded in a capturing stream")
                import time
                self.dist.wait(self.__dict__.pop("_ids_pending", None))
                torch.cuda.synchronize()
                time.sleep(0.25)
                g = torch.cuda.CUDAGraph()
                try:
                    with torch.cuda.graph(g, capture_error_mode="thread_local"):
                        for _, fns in seq:
                            for fn in fns:
                                fn()
                        # an exchange started for the NEXT step (look-ahead ids) has to be joined inside the graph that started it
                        self.dist.wait(self.__dict__.pop("_ids_pending", None))
                except Exception as e:  # noqa: BLE001
                    import warnings
                    warnings.warn(f"hipGraph capture of the whole data-parallel step failed ({e}); falling back to launch segments")
                    torch.cuda.synchronize()
                    self._one_graph_ok = False
                    self.__dict__.pop("_ids_pending", None)
                    g = None
                    # the sequences were built with a side chain, which launch segments cannot hold: build them again without
                    self._dp_seq = None
                    self._dp_seqs.clear()
                    seq = sequence()
                else:
                    if self._one_graph_ok is None:
                        self._one_graph_ok = True
                        self.dist._on_close.append(self._drop_graphs)
                    self._step_graphs[key] = g
            if g is not None:
                g.replay()
                self._warm += 1
                return
        for i, (is_comm, fns) in enumerate(seq):
            if is_comm or not (self.use_graph and self._warm >= 2):
                for fn in fns:
                    fn()
                continue
            i = (key, i)
            g = self._stage_graphs.get(i)
            if g is None:
                # thread-local capture mode: the RCCL watchdog thread keeps querying events while we capture
                g = torch.cuda.CUDAGraph()
                try:
                    with torch.cuda.graph(g, capture_error_mode="thread_local"):
                        for fn in fns:
                            fn()
                except Exception as e:  # noqa: BLE001  (capture refused: run this and every later segment eagerly)
                    import warnings
                    warnings.warn(f"hipGraph capture of launch segment {i} failed ({e}); continuing without graphs")
                    torch.cuda.synchronize()
                    self.use_graph = False
                    self._stage_graphs.clear()
                    for fn in fns:
                        fn()
                    continue
                self._stage_graphs[i] = g
            g.replay()
        self._warm += 1

    def _row_weight(self, weight):
        """step()'s weight= against what the step was built with, before anything is staged -> the flat fp32 row weights or None"""
        lw = self.loss_weights
        if weight is None:
            if lw is not None and lw.row:
                raise ValueError("this TrainStep was built with LossWeights(row=True): step(...) needs weight=")
            return None
        if lw is None:
            raise ValueError("weight= given to a TrainStep built without loss_weights")
        if not lw.row:
            raise ValueError("weight= given to a TrainStep whose LossWeights has row=False")
        row = weight.reshape(-1)
        if not (row.is_cuda and row.dtype == torch.float32 and row.numel() == self.B):
            raise ValueError(f"weight must be fp32 [{self.B}] or [{self.B},1] on the device")
        return row.contiguous()

    def _stage_weights(self, row):
        """the step's effective row weights into the static buffer: one eager launch, after the batch has been staged (it reads the
        staged ids and labels), no host synchronisation"""
        lw = self.loss_weights
        if lw is None:
            return
        dw = self._domain_w
        L.launch("cdc_stage_weights", self.lib.cdc_stage_weights,
                 (None if row is None else row.data_ptr(), self.emb.ids.data_ptr(), self.emb.F, 0 if dw is None else lw.domain_idx,
                  None if dw is None else dw.data_ptr(), 0 if dw is None else dw.numel(), self.y.data_ptr(), lw.pos_weight,
                  self.w.data_ptr(), self.B), C.c_void_p(torch.cuda.current_stream().cuda_stream))

    def step(self, X, y, group=None, next_X=None, *, weight=None):
        """One training step. X int32 [B,F]; y int16/float [B] or [B,1]; group int64 [B] or [B,1] (multi mode).
        next_X (optional): the ids of the batch the NEXT call will be given (device int32 [B,F], not modified until then) — with the
        look-ahead sort (_ahead_ok; data parallel: _ahead_dp_ok) its rows are sorted beside this step's forward/backward; a next call
        with another tensor simply sorts its own.  weight (required iff the step was built with LossWeights(row=True)): fp32 [B] or
        [B,1] on the device, this batch's per-row loss weights.  Returns (bce_loss, reg_loss) as device tensors (no host
        synchronisation)."""
        row_w = self._row_weight(weight)
        gdst = self.group if self.group is not None else (self.group_in if self.mode == "single_group" else None)
        yf = y.reshape(-1)
        gf = None if (group is None or gdst is None) else group.reshape(-1)
        fast = (X.is_cuda and X.dtype == torch.int32 and X.is_contiguous() and tuple(X.shape) == (self.B, self.emb.F) and
                yf.is_cuda and yf.dtype == torch.int16 and yf.is_contiguous() and yf.numel() == self.B and
                (gdst is None or (gf is not None and gf.is_cuda and gf.dtype == torch.int64 and gf.is_contiguous() and gf.numel() == self.B)))
        if not self._reg_checked or (self.opt.table_mode == "lazy" and not self.opt.table_reg_ready):
            # the first reported loss of a lazy run carries the table's L2 term like every later one (a freshly built or LOADED
            # optimiser has not evaluated it yet: load_state_dict clears table_reg_ready, also for a TrainStep that already ran).
            # Before the staging launch: that launch may advance the step counter (_stage_begins), and the refresh brings the
            # table to the counter's step
            self._reg_checked = True
            if self.opt.table_mode == "lazy" and not self.opt.table_reg_ready:
                self.refresh_table_reg()
        nx = None
        if fast and self._stage_begins:                           # + begin_step, + the next batch's ids for the look-ahead sort
            if ((self._ahead_ok or self._ahead_dp_ok) and next_X is not None and next_X.is_cuda and next_X.dtype == torch.int32 and
                    next_X.is_contiguous() and tuple(next_X.shape) == (self.B, self.emb.F)):
                nx = next_X
            L.launch("cdc_stage_batch", self.lib.cdc_stage_batch_next,
                     (X.data_ptr(), yf.data_ptr(), None if gdst is None else gf.data_ptr(), self.emb.ids.data_ptr(), self.y.data_ptr(),
                      None if gdst is None else gdst.data_ptr(), self.B, self.emb.F, None if nx is None else nx.data_ptr(),
                      None if nx is None else self.ids_next.data_ptr(), self.opt.step_dev.data_ptr(), self.opt.reg_sum.data_ptr(), 2,
                      self.field_dims_dev.data_ptr(), self.alias.data_ptr()),
                     C.c_void_p(torch.cuda.current_stream().cuda_stream))
        elif fast:                                                # one launch instead of three copies
            L.launch("cdc_stage_batch", self.lib.cdc_stage_batch,
                     (X.data_ptr(), yf.data_ptr(), None if gdst is None else gf.data_ptr(), self.emb.ids.data_ptr(), self.y.data_ptr(),
                      None if gdst is None else gdst.data_ptr(), self.B, self.emb.F, self.field_dims_dev.data_ptr(), self.alias.data_ptr()),
                     C.c_void_p(torch.cuda.current_stream().cuda_stream))
        else:
            self.emb.ids.copy_(X)
            bad = ((self.emb.ids < 0) | (self.emb.ids >= self.field_dims_dev)).reshape(-1).to(torch.int32)
            torch.maximum(self.alias, (bad * torch.arange(1, bad.numel() + 1, device=bad.device, dtype=torch.int32)).max().reshape(1), out=self.alias)
            self.y.copy_(yf)
            if gdst is not None:
                gdst.copy_(gf)
            if self._stage_begins:
                self.opt.begin_step()
        self._stage_weights(row_w)
        if self.dp_on:
            self._step_dp(X if fast else None, nx)
            return self.loss, self.reg
        key = self._lookahead(X if fast else None, nx)
        if self.use_graph and self._warm >= 2:
            g = self._graphs.get(key)
            if g is None:
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    self._launch(*key)
                self._graphs[key] = self.graph = g
            g.replay()
        else:
            self._launch(*key)
            self._warm += 1
        return self.loss, self.reg

    def profile(self, batches, n_steps=10, skip=2, overlap=True):
        """Per-launch timing of `n_steps` eager steps (HIP events on the stream each launch goes to); the first `skip` are not
        counted.  Returns {name: {"ms_per_step", "launches_per_step", "flops_per_step", "bytes_per_step"}}.  Events are read back
        and released every few steps: the runtime backs each timed event with a signal from a bounded pool.
        overlap=False: the whole step on one stream (the main stream is the side chain), i.e. every kernel's duration with the chip
        to itself."""
        was_graph, self.use_graph = self.use_graph, False
        was_overlap, self._overlap_ok = self._overlap_ok, bool(self._overlap_ok and overlap)
        self._per_launch_timing = not overlap
        rec = []
        out = {}
        used = max(n_steps - skip, 1)

        def fold(count):
            torch.cuda.synchronize()
            if count:
                for name, e0, e1, fl, nb in rec:
                    d = out.setdefault(name, {"ms_per_step": 0.0, "launches_per_step": 0.0, "flops_per_step": 0.0, "bytes_per_step": 0.0})
                    d["ms_per_step"] += e0.elapsed_time(e1) / used
                    d["launches_per_step"] += 1.0 / used
                    d["flops_per_step"] += fl / used
                    d["bytes_per_step"] += nb / used
            rec.clear()

        L.PROFILE = rec
        try:
            for i in range(n_steps):
                if i == skip:
                    fold(False)
                self.step(*batches[i % len(batches)])
                if i >= skip and (i - skip) % 4 == 3:
                    fold(True)
            fold(n_steps > skip)
        finally:
            L.PROFILE = None
            self.use_graph = was_graph
            self._overlap_ok = was_overlap
            self._per_launch_timing = False
        return out

    def sibling(self, batch_size, global_rows=None, cap_rows=None):
        """A TrainStep for another batch size on the SAME model and optimiser state (the ragged last batch of an epoch,
        which the reference trains on like any other: run.py:476); runs eagerly.  Data parallel: batch_size is THIS rank's share
        of the ragged global batch, global_rows its true size, cap_rows the largest share (ceil(global_rows / world)); every rank
        must call it (the step's collectives).  Row-sharded table, or equal shares with the replicated one."""
        key = (int(batch_size), None if global_rows is None else int(global_rows), None if cap_rows is None else int(cap_rows))
        sib = self.__dict__.setdefault("_siblings", {})
        ts = sib.get(key)
        if ts is None:
            if self.world > 1:
                if global_rows is None or cap_rows is None:
                    raise ValueError("a ragged batch under data parallelism needs global_rows and cap_rows (data.train_epoch passes them)")
                if self.table_dist != "sharded" and int(global_rows) != int(batch_size) * self.world:
                    raise NotImplementedError("uneven shares of a ragged batch need the row-sharded table (the replicated table's "
                                              "all-gathers are equal-sized)")
                ts = TrainStep(self.model, self.opt, int(batch_size), mode=self.mode, use_graph=False, dist=self.dist, sync_bn=self.sync_bn,
                               table_dist=self.table_dist, shard_slack=self._shard_slack, train_mode=self.train_mode, sort_ahead=False,
                               global_rows=int(global_rows), cap_rows=int(cap_rows), loss_weights=self.loss_weights)
            else:
                ts = TrainStep(self.model, self.opt, int(batch_size), mode=self.mode, use_graph=False, train_mode=self.train_mode,
                               loss_weights=self.loss_weights)
            sib[key] = ts
        return ts

    def check_ids(self):
        """Host-synchronising: raises IndexError like the reference if the last batch held an out-of-range id."""
        bad = int(self.emb.err.item())
        if bad:
            self.emb.err.zero_()
            self.alias.zero_()
            raise IndexError(f"index out of range in self (flat position {bad - 1})")
        al = int(self.alias.item())
        if al:
            self.alias.zero_()
            b, f = divmod(al - 1, self.emb.F)
            raise ValueError(f"the id at batch position {b}, field {f} lies outside the field's vocabulary but inside the table: it aliases a row "
                             "of another field.  The reference trains that row through both fields at once (one Adam update of the summed "
                             "gradient, model/layer.py:152-153); the per-field row lists of this path update it once per field, so the "
                             "results of that step are not the reference's")
        for op in self.plan.ops:                                  # in-launch exchanges that gave up (csrc/tower.hip)
            word = getattr(op, "tmo_word", None)
            if torch.is_tensor(word) and int(word.item()) & L.TOWER_ERR_TIMEOUT:
                word.zero_()
                getattr(op, "ws").zero_()
                raise RuntimeError("the fused tower launch timed out waiting for its other workgroups (BatchNorm statistics "
                                   "exchange); the results of that step are void")
        if self.dp_on and self.table_dist == "sharded":
            over = int(self.overflow.item())
            if over:
                self.overflow.zero_()
                raise RuntimeError(f"row-sharded table: a per-owner row list needed {over} slots but holds {self.cap}; "
                                   f"raise shard_slack (rows beyond the capacity were dropped from that step)")
