"""load_vocabulary and the learning-rate schedules of the reference's clickstream_transformer/training_utils.py (:5-59).
The schedules are host Python: float64 arithmetic on the step number, a Python float out.  optim.Adam(learning_rate=<schedule>)
calls one with the number of optimizer steps already taken (0 at the first step), as Keras calls a LearningRateSchedule.
The Keras callbacks of that file (SavedModel export, TensorBoard) are outside the hot path."""
import math
import os


def load_vocabulary(vocab_file):
    """Lines of the vocabulary file, stripped.  A directory raises IsADirectoryError as the reference does."""
    if os.path.isdir(vocab_file):
        raise IsADirectoryError('%s is a directory.' % vocab_file)
    with open(vocab_file, 'r') as f:
        return [ln.strip() for ln in f.readlines()]


class CustomLRSchedule:
    """The "Attention is all you need" warm-up of the reference (training_utils.py:15-36):
        lr(step) = d_model^-1/2 * min(step^-1/2, step * warmup_steps^-3/2) * scale * scale
    with the reference's two quirks kept: `scale` is applied twice (:34 and :36), and step 0 gives min(inf, 0) = 0, so the first
    optimizer step moves nothing."""

    def __init__(self, d_model, warmup_steps=4000, scale=1):
        self.d_model = float(d_model)
        self.warmup_steps = warmup_steps
        self.scale = scale

    def get_config(self):
        return {'d_model': self.d_model, 'warmup_steps': self.warmup_steps, 'scale': self.scale}

    def __call__(self, step):
        step = float(step)
        decay = 1.0 / math.sqrt(step) if step > 0.0 else math.inf
        warm = step * float(self.warmup_steps) ** -1.5
        return (1.0 / math.sqrt(self.d_model)) * min(decay, warm) * self.scale * self.scale


class CustomExponentialDecayLR:
    """Exponential decay towards a floor (training_utils.py:39-59):
        lr(step) = (initial - limiting) * decay_rate^(step / decay_steps) + limiting"""

    def __init__(self, initial_learning_rate, limiting_learning_rate, decay_steps, decay_rate):
        self.initial_learning_rate = initial_learning_rate
        self.limiting_learning_rate = limiting_learning_rate
        self.decay_steps = decay_steps
        self.decay_rate = decay_rate

    def get_config(self):
        return {'init_lr': self.initial_learning_rate, 'limit_lr': self.limiting_learning_rate, 'decay_steps': self.decay_steps,
                'decay_rate': self.decay_rate}

    def __call__(self, step):
        span = float(self.initial_learning_rate) - float(self.limiting_learning_rate)
        return span * float(self.decay_rate) ** (float(step) / float(self.decay_steps)) + float(self.limiting_learning_rate)


class WarmupLinearDecay:
    """NO REFERENCE ORACLE (an extension, like feature_combine='sum'): the BERT4Rec paper's shape -- linear warm-up from 0 to
    `peak_lr` over `warmup_steps` steps, then linear decay to `end_lr` at `total_steps`, constant after that:
        step <  warmup_steps:  peak_lr * step / warmup_steps
        step >= warmup_steps:  end_lr + (peak_lr - end_lr) * max(0, total_steps - step) / (total_steps - warmup_steps)"""

    def __init__(self, peak_lr, warmup_steps, total_steps, end_lr=0.0):
        if not 0 <= warmup_steps < total_steps:
            raise ValueError('WarmupLinearDecay needs 0 <= warmup_steps < total_steps, got %r and %r' % (warmup_steps, total_steps))
        self.peak_lr, self.warmup_steps, self.total_steps, self.end_lr = peak_lr, warmup_steps, total_steps, end_lr

    def get_config(self):
        return {'peak_lr': self.peak_lr, 'warmup_steps': self.warmup_steps, 'total_steps': self.total_steps, 'end_lr': self.end_lr}

    def __call__(self, step):
        step = float(step)
        peak, end = float(self.peak_lr), float(self.end_lr)
        if step < self.warmup_steps:
            return peak * step / float(self.warmup_steps)
        left = max(0.0, float(self.total_steps) - step)
        return end + (peak - end) * left / float(self.total_steps - self.warmup_steps)
