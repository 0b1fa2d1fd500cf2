"""Pure-Python restatement of the loss scaler's state machine (csrc/loss_scale.hip,
loss_scale_update_kernel): the rule of torch.amp.GradScaler plus the bookkeeping the update kernels
need.  Scales are float32 values (numpy), counters plain ints.  A plain helper module: the CPU test
checks it against hand-computed sequences (and torch's own kernel where this build has a CPU form),
the GPU test checks the device kernel against it, field by field."""
import numpy as np


class ScalerState:
    FIELDS = ('scale', 'inv_scale', 'skip', 'growth_tracker', 'steps', 'skipped', 'found')

    def __init__(self, init_scale=2.0 ** 16, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000):
        self.growth = np.float32(growth_factor)
        self.backoff = np.float32(backoff_factor)
        self.interval = int(growth_interval)
        self.scale = np.float32(init_scale)
        self.inv_scale = np.float32(1.0 / float(np.float32(init_scale)))
        self.skip = 0
        self.growth_tracker = 0
        self.steps = 0
        self.skipped = 0
        self.found = 0

    def update(self, found):
        """one step: `found` = a scan saw a non-finite gradient"""
        self.found = 1 if found else 0
        used = self.scale
        # the reciprocal of the scale THIS step's gradients carry (double division, rounded once)
        self.inv_scale = np.float32(1.0 / float(used))
        self.steps += 1
        if self.found:
            self.scale = np.float32(used * self.backoff)
            self.growth_tracker = 0
            self.skip = 1
            self.skipped += 1
        else:
            self.skip = 0
            t = self.growth_tracker + 1
            if t == self.interval:
                with np.errstate(over='ignore'):
                    grown = np.float32(used * self.growth)
                if np.isfinite(grown):
                    self.scale = grown            # else: the growth is not applied
                t = 0
            self.growth_tracker = t
        self.found = 0
        return self

    def fields(self):
        return {k: (float(getattr(self, k)) if k in ('scale', 'inv_scale') else int(getattr(self, k)))
                for k in self.FIELDS}
