"""mx.lr_scheduler: the base class the reference's lib/utils/lr_scheduler.py derives from (MXNet v1.1.0
python/mxnet/lr_scheduler.py): a `base_lr` attribute, which the optimizer overwrites with its learning rate, and
__call__(num_update) -> learning rate."""


class LRScheduler(object):
    def __init__(self, base_lr=0.01):
        self.base_lr = base_lr

    def __call__(self, num_update):
        raise NotImplementedError("must override this")
