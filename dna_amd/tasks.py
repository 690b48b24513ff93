"""Task / loss / metric glue of the MLM path (reference src/tasks/*).

  bert_cross_entropy   src/tasks/metrics.py:268-273  (registered as output_metric_fns name)
  LMTask / HG38Task    src/tasks/tasks.py:169-191, :254-339 (identity encoder/decoder,
                       flatten logits, loss by name); registry "lm", "hg38"
  Perplexity, NumTokens  src/tasks/torchmetrics.py:24-115 (state kept as tensors; the
                       distributed reduction is a SUM all-reduce, like dist_reduce_fx="sum")
"""
import math

import torch
import torch.nn.functional as F


def bert_cross_entropy(x, y):
    """CE over the masked positions: x = (logits [(b*S), V], mask [b, S]), y = target ids."""
    logits = x[0]
    mask = x[1].reshape(y.shape)
    return F.cross_entropy(logits[mask], y[mask])


def cross_entropy(logits, y, ignore_index=-100):
    logits = logits.view(-1, logits.shape[-1])
    return F.cross_entropy(logits, y.view(-1), ignore_index=ignore_index)


output_metric_fns = {"bert_cross_entropy": bert_cross_entropy, "cross_entropy": cross_entropy}


class Perplexity:
    """exp(sum(loss * count) / sum(count)) accumulated in float64 (torchmetrics.py:24-73)."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.total_log_probs = torch.zeros((), dtype=torch.float64)
        self.count = torch.zeros((), dtype=torch.int64)

    def update(self, preds, target, loss):
        self.update_count(loss, target.numel())

    def update_count(self, loss, count):
        """update() given target.numel() instead of the target tensor (no device sync)."""
        self.total_log_probs = self.total_log_probs.to(loss.device) + loss.detach().double() * count
        self.count = self.count.to(loss.device) + count

    def compute(self):
        return torch.exp(self.total_log_probs / self.count)


class NumTokens:
    """Running count of target tokens, never reset between epochs (torchmetrics.py:75-115)."""

    def __init__(self):
        self.count = torch.zeros((), dtype=torch.int64)

    def reset(self):
        pass

    def update(self, preds, target, loss=None):
        self.count = self.count + target.numel()

    def compute(self):
        return self.count


class ConfusionMatrix:
    """[C, C] int64 counts (rows: label, columns: prediction) accumulated on the device of the
    inputs -- no host sync per batch -- from the head's `pred` and the labels. compute() at epoch
    end gives accuracy, the multi-class Matthews correlation coefficient and macro F1 over the
    pooled predictions of the epoch (what the GUE tables report; equal to
    sklearn.metrics.matthews_corrcoef / f1_score(average="macro") on them). The reference calls
    sklearn per batch instead and averages the per-batch values (src/tasks/metrics.py:83-87,
    :229-233).

    per_class: which of PER_CLASS compute() adds -- lists in class order, a class that never
    occurs (as a label for accuracy / recall, as a prediction for precision) reported as 0. The
    reference's species experiment names them in task.metrics and defines none of them; here
    accuracy_per_class is the fraction of a class's sequences that are classified as it, which
    for one label per sequence is its recall."""

    PER_CLASS = ("accuracy_per_class", "precision_per_class", "recall_per_class")

    def __init__(self, num_classes, per_class=()):
        self.num_classes = int(num_classes)
        self.per_class = tuple(m for m in self.PER_CLASS if m in tuple(per_class))
        self.reset()

    def reset(self):
        self.counts = torch.zeros(self.num_classes, self.num_classes, dtype=torch.int64)

    def update(self, pred, target):
        """counts[target, pred] += 1 for every pair: an index_add_ into the preallocated matrix,
        which reads nothing back to the host (torch.bincount would, to size its output). Labels
        and predictions must lie in [0, num_classes); that is not checked here, for the same
        reason."""
        C = self.num_classes
        idx = target.reshape(-1).to(torch.int64) * C + pred.reshape(-1).to(torch.int64)
        if self.counts.device != idx.device:  # once: the matrix moves to where the batches are
            self.counts = self.counts.to(idx.device)
        self.counts.view(-1).index_add_(0, idx, torch.ones_like(idx))

    def compute(self):
        m = self.counts.to(torch.float64).cpu()
        n = m.sum()
        tp = m.diag()
        t, p = m.sum(1), m.sum(0)  # per class: how often it is the label / the prediction
        acc = (tp.sum() / n).item() if n > 0 else 0.0
        # Gorodkin's R_K, as sklearn.metrics.matthews_corrcoef
        cov_tp = tp.sum() * n - (t * p).sum()
        cov_pp = n * n - (p * p).sum()
        cov_tt = n * n - (t * t).sum()
        den = cov_pp * cov_tt
        mcc = (cov_tp / den.sqrt()).item() if den > 0 else 0.0
        # macro F1 over the classes that occur as a label or a prediction (sklearn's label set);
        # a class with no true positive scores 0
        present = (t + p) > 0
        f1 = torch.where(tp > 0, 2 * tp / (t + p).clamp(min=1), torch.zeros_like(tp))
        f1_macro = f1[present].mean().item() if present.any() else 0.0
        out = {"accuracy": acc, "mcc": mcc, "f1_macro": f1_macro}
        ratio = lambda den: torch.where(den > 0, tp / den.clamp(min=1), torch.zeros_like(tp)).tolist()
        for name in self.per_class:
            out[name] = ratio(p if name == "precision_per_class" else t)
        return out


class PearsonR:
    """Pearson correlation per target column from float64 running sums (n, sum x, sum y, sum x^2,
    sum y^2, sum xy per column), accumulated on the device of the inputs -- no host sync per
    batch. compute() at the end of a split gives pearsonr_<name> per column and pearsonr_mean
    over the pooled predictions of the split. The reference calls scipy.stats.pearsonr per batch
    instead and averages the per-batch values (src/tasks/metrics.py:326-352)."""

    def __init__(self, names=("dev", "hk")):
        self.names = tuple(names)
        self.reset()

    def reset(self):
        self.sums = torch.zeros(6, len(self.names), dtype=torch.float64)

    def update(self, pred, target):
        """pred, target [b, len(names)] (target in any shape with as many values)."""
        x = pred.detach().reshape(-1, len(self.names)).to(torch.float64)
        y = target.detach().reshape(x.shape).to(torch.float64)
        if self.sums.device != x.device:  # once: the sums move to where the batches are
            self.sums = self.sums.to(x.device)
        self.sums += torch.stack([torch.ones_like(x).sum(0), x.sum(0), y.sum(0), (x * x).sum(0),
                                  (y * y).sum(0), (x * y).sum(0)])

    def compute(self):
        n, sx, sy, sxx, syy, sxy = self.sums.cpu()
        cov = n * sxy - sx * sy
        den = ((n * sxx - sx * sx) * (n * syy - sy * sy)).clamp(min=0).sqrt()
        r = torch.where(den > 0, cov / den.clamp(min=1e-300), torch.zeros_like(cov))
        out = {f"pearsonr_{name}": v for name, v in zip(self.names, r.tolist())}
        out["pearsonr_mean"] = r.mean().item() if len(self.names) else 0.0
        return out


class MultilabelAUROC:
    """Area under the ROC curve per label, averaged over the labels (the DeepSEA paper's metric).
    update() keeps the batch's logits (fp32) and labels (uint8) on the device of the inputs -- no
    host sync per batch; compute() at the end of a split ranks each label's logits over the
    pooled predictions of the split (average ranks on ties) and takes the rank-sum (Mann-Whitney)
    AUROC: (sum of the positives' ranks - n_pos (n_pos + 1) / 2) / (n_pos n_neg). -> `roc`, the
    mean over the labels for which both classes occur, and `roc_labels_skipped`, how many labels
    had only one class.

    Not the reference's `roc` (src/tasks/metrics.py:251-279), which softmaxes the logits across
    the labels, scores the flattened [batch x labels] values as one binary problem with sklearn,
    per batch, and averages the per-batch values."""

    def __init__(self, num_labels):
        self.num_labels = int(num_labels)
        self.reset()

    def reset(self):
        self.logits, self.labels = [], []

    def update(self, logits, target):
        self.logits.append(logits.detach().reshape(-1, self.num_labels).to(torch.float32))
        self.labels.append((target.detach().reshape(-1, self.num_labels) > 0.5).to(torch.uint8))

    def compute(self):
        if not self.logits:
            return {"roc": 0.0, "roc_labels_skipped": self.num_labels}
        x = torch.cat(self.logits).to(torch.float64)
        y = torch.cat(self.labels).to(torch.float64)
        n = x.shape[0]
        xs, order = x.sort(dim=0, stable=True)
        # average rank of a run of ties: (first + last 1-based position of the run) / 2
        pos = torch.arange(1, n + 1, dtype=torch.float64, device=x.device)[:, None].expand_as(xs)
        new = torch.ones_like(xs, dtype=torch.bool)
        new[1:] = xs[1:] != xs[:-1]
        first = torch.where(new, pos, torch.zeros_like(pos)).cummax(dim=0).values
        last_of_run = torch.ones_like(new)
        last_of_run[:-1] = new[1:]
        big = torch.full_like(pos, float(n + 1))
        last = torch.where(last_of_run, pos, big).flip(0).cummin(dim=0).values.flip(0)
        ys = y.gather(0, order)
        n_pos = ys.sum(0)
        n_neg = n - n_pos
        u = (ys * (first + last) / 2).sum(0) - n_pos * (n_pos + 1) / 2
        ok = (n_pos > 0) & (n_neg > 0)
        auc = u / (n_pos * n_neg).clamp(min=1)
        skipped = int((~ok).sum().item())
        roc = auc[ok].mean().item() if skipped < self.num_labels else 0.0
        return {"roc": roc, "roc_labels_skipped": skipped}


# task.loss of a pooling-head experiment -> (the head's problem type, what the head's loss -- a
# mean over B x C -- is multiplied by). customMSE (reference metrics.py:354-356) is the sum over
# the C columns of each column's mean: C times the head's loss. deepsea_loss is
# binary_cross_entropy under another name (metrics.py:282-285).
POOL_LOSSES = {
    "cross_entropy": ("single_label_classification", lambda c: 1.0),
    "mse": ("regression", lambda c: 1.0),
    "customMSE": ("regression", lambda c: float(c)),
    "binary_cross_entropy": ("multi_label_classification", lambda c: 1.0),
    "deepsea_loss": ("multi_label_classification", lambda c: 1.0),
}
# task._name_ -> the problem type its losses must have and its default loss
POOL_TASKS = {
    "sequence_classification": ("single_label_classification", "cross_entropy"),
    # the reference's Nucleotide Transformer experiments name their task masked_multiclass; with
    # one label per sequence and cross_entropy it is the single-label task above
    "masked_multiclass": ("single_label_classification", "cross_entropy"),
    "regression": ("regression", "mse"),
    "multilabel_classification": ("multi_label_classification", "binary_cross_entropy"),
}


def pool_loss(task_name, loss_name, num_labels):
    """-> (problem_type, loss_scale) of a pooling-head task; an unknown task or loss, or a loss
    of another task's kind, is a ValueError that names it."""
    if task_name not in POOL_TASKS:
        raise ValueError(f"task._name_={task_name!r}: one of {sorted(POOL_TASKS)}")
    problem, default = POOL_TASKS[task_name]
    loss_name = default if loss_name is None else loss_name
    if loss_name not in POOL_LOSSES:
        raise ValueError(f"task.loss={loss_name!r}: one of {sorted(POOL_LOSSES)}")
    kind, scale = POOL_LOSSES[loss_name]
    if kind != problem:
        raise ValueError(f"task.loss={loss_name!r} is a {kind} loss; task._name_={task_name!r} "
                         f"needs a {problem} one")
    return problem, scale(num_labels)


torchmetric_fns = {"perplexity": Perplexity, "num_tokens": NumTokens}


class LMTask:
    """forward(batch, model) -> (x, y, w) exactly like LMTask.forward (tasks.py:169-191) with
    identity encoder/decoder (encoder: null, decoder: null in configs/pipeline/bert_hg38.yaml)."""

    def __init__(self, dataset=None, model=None, loss="cross_entropy", torchmetrics=None,
                 metrics=None, **unused):
        name = loss if isinstance(loss, str) else loss["_name_"]
        self.loss_name = name
        self.loss = output_metric_fns[name]
        self.torchmetric_names = list(torchmetrics or [])
        self.train_torchmetrics = {n: torchmetric_fns[n]() for n in self.torchmetric_names}

    def forward(self, batch, model, state=None):
        x, y = batch[0], batch[1]
        out, state = model(x, state=state)
        logits = out.logits
        if isinstance(logits, tuple):
            logits = list(logits)
            logits[0] = logits[0].reshape(-1, logits[0].shape[-1])
        else:
            logits = logits.reshape(-1, logits.shape[-1])
        return logits, y.reshape(-1), {}


class HG38Task(LMTask):
    pass


registry = {"lm": LMTask, "hg38": HG38Task}
