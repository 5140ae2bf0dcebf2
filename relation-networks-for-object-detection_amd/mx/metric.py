"""mx.metric: the evaluation-metric protocol of MXNet v1.1.0 (python/mxnet/metric.py) as far as the reference's
core/metric.py and train_end2end.py use it: EvalMetric (name, num_inst, sum_metric, reset, get, get_name_value, update_dict)
and CompositeEvalMetric (add, get_metric, update, reset, get).  Host-side bookkeeping only."""


class EvalMetric(object):
    def __init__(self, name, output_names=None, label_names=None, **kwargs):
        self.name = str(name)
        self.output_names, self.label_names = output_names, label_names
        self._kwargs = kwargs
        self.reset()

    def __str__(self):
        return "EvalMetric: {}".format(dict(self.get_name_value()))

    def update_dict(self, label, pred):
        pred = [pred[n] for n in self.output_names] if self.output_names is not None else list(pred.values())
        label = [label[n] for n in self.label_names] if self.label_names is not None else list(label.values())
        self.update(label, pred)

    def update(self, labels, preds):
        raise NotImplementedError()

    def reset(self):
        self.num_inst = 0
        self.sum_metric = 0.0

    def get(self):
        if self.num_inst == 0:
            return (self.name, float('nan'))
        return (self.name, self.sum_metric / self.num_inst)

    def get_name_value(self):
        name, value = self.get()
        if not isinstance(name, list):
            name = [name]
        if not isinstance(value, list):
            value = [value]
        return list(zip(name, value))


class CompositeEvalMetric(EvalMetric):
    """Several metrics updated together; get() concatenates their names / values in registration order."""

    def __init__(self, metrics=None, name='composite', output_names=None, label_names=None):
        super(CompositeEvalMetric, self).__init__(name, output_names=output_names, label_names=label_names)
        self.metrics = list(metrics) if metrics is not None else []

    def add(self, metric):
        self.metrics.append(metric)

    def get_metric(self, index):
        try:
            return self.metrics[index]
        except IndexError:
            return ValueError("Metric index {} is out of range 0 and {}".format(index, len(self.metrics)))

    def update_dict(self, labels, preds):
        for metric in self.metrics:
            metric.update_dict(labels, preds)

    def update(self, labels, preds):
        for metric in self.metrics:
            metric.update(labels, preds)

    def reset(self):
        for metric in getattr(self, 'metrics', []):
            metric.reset()

    def get(self):
        names, values = [], []
        for metric in self.metrics:
            name, value = metric.get()
            names.extend(name if isinstance(name, list) else [name])
            values.extend(value if isinstance(value, list) else [value])
        return (names, values)
