"""Two numpy statements of the global feature statistics, shared by the stats tests.  Test infrastructure: the product never imports this.

* ``ReferenceStatement`` -- the arithmetic of ``StatsAccumulator`` (lhotse/features/base.py:990-1033) in this project's words: one
  float64 update per cut.  tests/test_stats_golden.py holds it to the reference's own results bit for bit; it is what the device is
  measured against.
* ``DeviceStatement`` -- the blocked order of csrc/kernel_stats.hpp (blocks of ``BLOCK_FRAMES`` frames, 16 row lanes, the pairwise merge
  in block order, then the same update).  It serves to DERIVE expectations (and stands in for the handle where there is no device); it
  is never a bar for the device.

``truth`` is the longdouble answer over the concatenated inputs and ``errors`` the two error figures of the bar."""
import numpy as np

BLOCK_FRAMES = 256  # kStBlockFrames
ROW_LANES = 16      # kStRowLanes


def _update(total_frames, total_sum, total_var, n, s, m2):
    """The running totals with one more matrix of ``n`` frames (sum ``s``, unnormalised variance ``m2``), operation for operation."""
    with np.errstate(all="ignore"):
        if total_frames > 0:
            ratio = total_frames / n
            total_var = total_var + m2 + ratio / (total_frames + n) * (total_sum / ratio - s) ** 2
        else:
            total_var = m2
        return total_frames + n, total_sum + s, total_var


class ReferenceStatement:
    def __init__(self, feature_dim):
        self.total_frames, self.total_sum, self.total_unnorm_var = 0, np.zeros(feature_dim), np.zeros(feature_dim)

    def update(self, arr):
        x = np.asarray(arr).astype(np.float64)
        with np.errstate(all="ignore"):
            n, s = x.shape[0], x.sum(axis=0)
            m2 = np.var(x, axis=0) * n
        self.total_frames, self.total_sum, self.total_unnorm_var = _update(self.total_frames, self.total_sum, self.total_unnorm_var, n, s, m2)

    def merge(self, other):
        if other.total_frames:
            self.total_frames, self.total_sum, self.total_unnorm_var = _update(self.total_frames, self.total_sum, self.total_unnorm_var, other.total_frames,
                                                                               other.total_sum, other.total_unnorm_var)

    @property
    def norm_means(self):
        return self.total_sum / self.total_frames

    @property
    def norm_stds(self):
        return np.sqrt(self.total_unnorm_var / self.total_frames)

    def get(self):
        return {"norm_means": self.norm_means, "norm_stds": self.norm_stds}


def _lanes_sum(x):
    """(n <= BLOCK_FRAMES, F) float64 -> (F,): lane r sums the frames r, r + 16, ... in order from 0.0, then the 16 lanes in order."""
    lanes = np.zeros((ROW_LANES, x.shape[1]))
    for k in range(0, len(x), ROW_LANES):
        rows = x[k: k + ROW_LANES]
        lanes[: len(rows)] = lanes[: len(rows)] + rows
    t = lanes[0].copy()
    for r in range(1, ROW_LANES):
        t = t + lanes[r]
    return t


class DeviceStatement(ReferenceStatement):
    def update(self, arr):
        x = np.asarray(arr).astype(np.float64)
        if len(x) == 0:
            return  # a cut of no frames contributes nothing
        with np.errstate(all="ignore"):
            n = s = m2 = None
            for f0 in range(0, len(x), BLOCK_FRAMES):
                blk = x[f0: f0 + BLOCK_FRAMES]
                nb, sb = len(blk), _lanes_sum(blk)
                mb = _lanes_sum((blk - sb / nb) ** 2)
                if n is None:
                    n, s, m2 = nb, sb, mb
                else:
                    delta = sb / nb - s / n
                    m2 = m2 + mb + delta * delta * (float(n) * float(nb) / float(n + nb))
                    n, s = n + nb, s + sb
        self.total_frames, self.total_sum, self.total_unnorm_var = _update(self.total_frames, self.total_sum, self.total_unnorm_var, n, s, m2)


def truth(matrices):
    """longdouble mean and std per bin over the concatenated (float32) inputs, two-pass."""
    x = np.concatenate([np.asarray(m) for m in matrices if len(m)]).astype(np.longdouble)
    mean = x.sum(axis=0) / len(x)
    std = np.sqrt(((x - mean) ** 2).sum(axis=0) / len(x))
    return mean, std, np.abs(x).mean(axis=0)


def errors(means, stds, matrices):
    """-> (mean error, std error): max over bins of |value - truth| / scale; scale = mean(|x|) of the bin for the mean, std for the std."""
    mean, std, mabs = truth(matrices)
    with np.errstate(all="ignore"):
        em = np.abs(np.asarray(means).astype(np.longdouble) - mean) / mabs
        es = np.abs(np.asarray(stds).astype(np.longdouble) - std) / std
    return float(np.nanmax(em)), float(np.nanmax(es))


GOLDEN_CASES = {  # name -> (F, keyword arguments of make_matrices); tools/make_golden_stats.py stores the reference's results for each
    "f1": (1, {}), "f3": (3, {}), "f80": (80, {}), "f257": (257, {}), "offset80": (80, {"offset": 1e4, "scale": 4e-3}), "half80": (80, {"half": True}),
}


def make_matrices(F, seed=0, offset=0.0, scale=1.0, block=BLOCK_FRAMES, half=False):
    if half:  # binary16 values: the same cuts rounded to binary16, with subnormals, the largest finite values and both zeros among them
        mats = [m.astype(np.float16) for m in make_matrices(F, seed + 7, block=block)]
        special = np.array([6e-8, -6e-8, 5.96e-8, 65504.0, -65504.0, 0.0, -0.0, 6.1e-5], dtype=np.float16)
        for i, m in enumerate(mats):
            if m.size >= len(special):
                m.reshape(-1)[i: i + len(special)] = special
        return mats
    return _make_matrices(F, seed, offset, scale, block)


def _make_matrices(F, seed, offset, scale, block):
    """The cuts of the GPU cases: 1, 2, block - 1, 0 (in the middle), block, block + 1 and 3 * block + 5 frames, log-mel-like float32
    (``offset``: values of ``offset + scale * N(0, 2.5)`` instead).  The reference statement is fed the cuts that have frames."""
    rng = np.random.RandomState(seed + 1000 * F)
    lens = [1, 2, block - 1, 0, block, block + 1, 3 * block + 5]
    return [(offset + scale * (rng.standard_normal((n, F)) * 2.5 - 8.0 * (offset == 0.0))).astype(np.float32) for n in lens]
