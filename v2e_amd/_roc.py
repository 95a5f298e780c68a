"""What `DenoiseResult`, `WindowResult` and `DoubleWindowResult` share: the rates of a `passed` array and their best setting."""
import numpy as np


class RocResult(object):
    """A result with `passed` (int64, one axis of which is the label: 1 = signal, 0 = noise), n_signal and n_noise.  LABEL_AXIS is
    that axis; tpr and fpr have passed's shape without it."""
    LABEL_AXIS = -2

    def _rate(self, label, n):
        p = np.take(self.passed, label, axis=self.LABEL_AXIS).astype(np.float64)
        return p / n if n > 0 else np.full(p.shape, np.nan)

    @property
    def tpr(self):
        return self._rate(1, self.n_signal)

    @property
    def fpr(self):
        return self._rate(0, self.n_noise)

    def _best(self, name):
        """(index, tpr, fpr) at the first maximum of tpr - fpr in C order, the index a tuple into tpr.  ValueError in the words of
        class `name` when tpr - fpr is NaN everywhere."""
        tpr, fpr = self.tpr, self.fpr
        d = (tpr - fpr).reshape(-1)
        if np.all(np.isnan(d)):
            raise ValueError("%s.best: needs at least one signal and one noise row" % name)
        at = np.unravel_index(int(np.nanargmax(d)), tpr.shape)  # (the first maximum in C order)
        return at, float(tpr[at]), float(fpr[at])
