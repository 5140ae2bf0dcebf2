"""The reference's learning-rate schedule (lib/utils/lr_scheduler.py:WarmupMultiFactorScheduler) and the way
train_end2end.py:154-161 sets it up from the configuration.

    sched = lr_scheduler.from_config(cfg.TRAIN, num_images=len(roidb), batch_size=batch)
    out = tr.forward_backward(*batch); tr.all_reduce(wait=False)
    tr.update(lr=sched(tr.step_count + 1))

Convention for `num_update`: MXNet's SGD increments its per-weight update count FIRST and then asks the scheduler
(Optimizer._update_count, then _get_lr), so the first update of a run is made with sched(1).  `Trainer.step_count` is the
number of updates already applied, hence `step_count + 1`.  (The optimizer is MXNet's, not part of the reference tree: this is
its documented behaviour, stated here rather than pinned.)
"""
import logging

from .mx.lr_scheduler import LRScheduler


class WarmupMultiFactorScheduler(LRScheduler):
    """base_lr * factor ** #(steps passed), with a constant warm-up rate first.

    step: increasing list of update counts (each >= 1); the rate drops once num_update is GREATER than a step.  While
    `warmup` and num_update < warmup_step the call returns warmup_lr and passes no step.  One call may pass several steps (a
    resumed run).  The object is stateful: `base_lr` holds the decayed rate, passed steps are not revisited."""

    def __init__(self, step, factor=1, warmup=False, warmup_lr=0, warmup_step=0):
        super(WarmupMultiFactorScheduler, self).__init__()
        assert isinstance(step, list) and len(step) >= 1
        for i, _step in enumerate(step):
            if i != 0 and step[i] <= step[i - 1]:
                raise ValueError("Schedule step must be an increasing integer list")
            if _step < 1:
                raise ValueError("Schedule step must be greater or equal than 1 round")
        if factor > 1.0:
            raise ValueError("Factor must be no more than 1 to make lr reduce")
        self.step, self.factor = step, factor
        self.cur_step_ind, self.count = 0, 0
        self.warmup, self.warmup_lr, self.warmup_step = warmup, warmup_lr, warmup_step

    def __call__(self, num_update):
        if self.warmup and num_update < self.warmup_step:
            return self.warmup_lr
        while self.cur_step_ind < len(self.step) and num_update > self.step[self.cur_step_ind]:
            self.count = self.step[self.cur_step_ind]
            self.cur_step_ind += 1
            self.base_lr *= self.factor
            logging.info("Update[%d]: Change learning rate to %0.5e", num_update, self.base_lr)
        return self.base_lr


def schedule_from_config(train_cfg, num_images, batch_size, begin_epoch=None):
    """-> (start rate, [update counts]) as train_end2end.py:154-159: `lr_step` is a comma-separated list of (fractional)
    epochs; the epochs at or before begin_epoch have already been applied (the start rate is decayed once for each of them), the
    others become int((epoch - begin_epoch) * num_images / batch_size) updates.  begin_epoch: default train_cfg.begin_epoch."""
    begin = train_cfg.begin_epoch if begin_epoch is None else begin_epoch
    lr_epoch = [float(e) for e in str(train_cfg.lr_step).split(',')]
    lr_epoch_diff = [e - begin for e in lr_epoch if e > begin]
    lr = train_cfg.lr * (train_cfg.lr_factor ** (len(lr_epoch) - len(lr_epoch_diff)))
    return lr, [int(e * num_images / batch_size) for e in lr_epoch_diff]


def from_config(train_cfg, num_images, batch_size, begin_epoch=None):
    """The scheduler of a training run, `base_lr` set to the (pre-decayed) start rate the way mx.optimizer sets it from its
    `learning_rate`.  train_cfg: cfg.TRAIN of config.py (lr, lr_step, lr_factor, warmup, warmup_lr, warmup_step, begin_epoch).
    Like the reference's class, a run with no step left after begin_epoch is refused (its assert on an empty list)."""
    lr, iters = schedule_from_config(train_cfg, num_images, batch_size, begin_epoch)
    sched = WarmupMultiFactorScheduler(iters, train_cfg.lr_factor, train_cfg.warmup, train_cfg.warmup_lr, train_cfg.warmup_step)
    sched.base_lr = lr
    return sched
