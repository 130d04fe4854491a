"""The epoch loop of the reference's driver on the HIP path: `Run.main` (run.py:713-770) with `Run.is_continuable`
(run.py:440-468) — train an epoch, evaluate on the validation set, keep the best checkpoint by `mean_auc` (falling back to
`total_auc` when no per-domain evaluation is configured), stop after `num_trials` epochs without improvement, reload the best
checkpoint and evaluate on the test set.  wandb logging, dataset preprocessing and model construction from `config` stay
with the caller (they are the reference's control plane: SURVEY §2).

`select_by="mean_gauc"` / `"total_gauc"` makes the per-user GAUC of an Evaluator with a user column (evaluate.py) the criterion
of both the best checkpoint and the early stop instead; `"mean_<fig>@<K>"` / `"total_<fig>@<K>"` with fig one of ndcg, recall,
precision, hit, mrr does the same with a per-user top-K figure of an Evaluator with `rank_at` (higher is better)."""
import re

import torch

from .data import train_epoch
from .evaluate import RANK_FIGURES, Evaluator

_RANK_KEY = re.compile(r"(?:mean|total)_(?:%s)@[1-9][0-9]*" % "|".join(RANK_FIGURES))


class Runner:
    def __init__(self, model, step, evaluator: Evaluator, save_model_path, num_trials=3, cdc_trainer=None, log=print, select_by=None):
        """step: the TrainStep (its optimiser is checkpointed); cdc_trainer: a CDCTrainer whose train_epoch replaces the
        plain epoch for CDC models (run.py:738-750).  select_by: None = the reference's rule (mean_auc, else total_auc);
        "mean_gauc" or "total_gauc" = that key of the evaluator's result; likewise "mean_<fig>@<K>" or "total_<fig>@<K>", a top-K
        figure (ndcg, recall, precision, hit, mrr) of an evaluator whose rank_at holds K."""
        if select_by not in (None, "mean_gauc", "total_gauc") and not (isinstance(select_by, str) and _RANK_KEY.fullmatch(select_by)):
            raise ValueError(f"select_by={select_by!r}: None, 'mean_gauc', 'total_gauc', or 'mean_<fig>@<K>' / 'total_<fig>@<K>' with fig "
                             f"one of {', '.join(RANK_FIGURES)}")
        self.select_by, self.best_select = select_by, 0.0
        self.model, self.step, self.evaluator = model, step, evaluator
        self.save_model_path, self.num_trials = save_model_path, int(num_trials)
        self.cdc_trainer, self.log = cdc_trainer, log
        self.best_auc = self.best_loss = self.best_mean_auc = self.best_mean_loss = 0.0
        self.trial_counter = 0

    def _sync_table(self):
        """every table row at the current step (and on every rank) before the parameters are read"""
        if getattr(self.step, "world", 1) > 1:
            self.step.gather_table()
        else:
            self.step.opt.flush_table()

    def _rank(self):
        d = getattr(self.step, "dist", None)
        return 0 if d is None else int(getattr(d, "rank", 0))

    def _barrier(self):
        d = getattr(self.step, "dist", None)
        if d is not None and getattr(self.step, "world", 1) > 1:
            d.barrier()

    def is_continuable(self, result_dict, epoch_i):
        score = result_dict.get("mean_auc")
        best = self.best_mean_auc
        if score is None:                       # is_evaluate_multi_domain off: the reference's commented-out total_auc criterion
            score, best = result_dict["total_auc"], self.best_auc
        if self.select_by is not None:
            if self.select_by not in result_dict and "@" in self.select_by:
                raise KeyError(f"select_by={self.select_by!r} but the evaluator's result has no such key: construct the Evaluator with "
                               f"user_idx (and n_user) and rank_at={self.select_by.split('@')[1]}"
                               + (", and per-domain evaluation for a mean_ figure" if self.select_by.startswith("mean_") else ""))
            if self.select_by not in result_dict:
                raise KeyError(f"select_by={self.select_by!r} but the evaluator's result has no such key: construct the Evaluator with "
                               f"user_idx (and n_user)" + (", and per-domain evaluation for mean_gauc" if self.select_by == "mean_gauc" else ""))
            score, best = result_dict[self.select_by], self.best_select
        if score > best:
            self.trial_counter = 0
            if self.select_by is not None:
                self.best_select = score
            self.best_auc, self.best_loss = result_dict["total_auc"], result_dict["total_loss"]
            save = {"epoch": epoch_i + 1, "state_dict": self.model.state_dict(), "best_auc": self.best_auc,
                    "best_result": result_dict, "optimizer": self.step.opt.state_dict()}
            if self.select_by is not None:
                save["select_by"], save["best_" + self.select_by] = self.select_by, score
            if result_dict.get("mean_auc") is not None:
                self.best_mean_auc, self.best_mean_loss = result_dict["mean_auc"], result_dict["mean_loss"]
                save["best_mean_auc"], save["best_mean_loss"] = self.best_mean_auc, self.best_mean_loss
            if hasattr(self.model, "domain2group_list"):
                save["domain2group_list"] = [int(v) for v in self.model.domain2group_list]
                save["s_group2domain_list"] = [[int(v) for v in g] for g in self.model.s_group2domain_list]
            if self._rank() == 0:                # one writer; the other ranks hold the same state after _sync_table()
                torch.save(save, self.save_model_path)
            self.log(f"current best epoch: {epoch_i + 1}, auc: {self.best_auc:.4f}, loss: {self.best_loss:.4f}")
            return True
        if self.trial_counter + 1 < self.num_trials:
            self.trial_counter += 1
            return True
        return False

    def fit(self, train_loader, valid_loader, test_loader=None, epochs=1):
        epoch_i = -1
        for epoch_i in range(epochs):
            if self.cdc_trainer is not None:
                self.cdc_trainer.train_epoch(epoch_i)
            else:
                self.model.train()
                train_epoch(self.step, train_loader)
            self._sync_table()
            result = self.evaluator.test(valid_loader)
            self.log(f"validation: auc: {result['total_auc']:.4f}, loss: {result['total_loss']:.4f}")
            if not self.is_continuable(result, epoch_i):
                break
        self._barrier()                          # rank 0's last save is complete before anyone reads it
        ck = torch.load(self.save_model_path, map_location=self.step.device, weights_only=False)     # our own file (result dicts inside)
        self.model.load_state_dict(ck["state_dict"])
        self.step.opt.load_state_dict(ck["optimizer"])
        out = {"epochs_run": epoch_i + 1, "best": ck["best_result"]}
        if test_loader is not None:
            out["test"] = self.evaluator.test(test_loader)
        return out
