"""Scenes for the tests of step 8 of the tracking rule (tests/test_smooth_host.py, tests/test_gpu_smooth.py): a rigid walker, exact and
noisy, and what the issue's conditions measure on it.  Plain NumPy, no import from the package under test."""
import numpy as np

J = 14
# integer offsets, extent 120 x 200 pixels: a figure 200 pixels tall, so the step-1 size s is 200
FIGURE = 2.0 * np.array([(-20, 40), (-20, 20), (-20, 0), (20, 0), (20, 20), (20, 40), (-30, -10), (-30, -30), (-20, -40), (20, -40),
                         (30, -30), (30, -10), (0, -45), (0, -60)], np.float64)
assert FIGURE[:, 1].max() - FIGURE[:, 1].min() == 200.0
TRACK = dict(max_misses=5, min_common=3, max_dist=0.05, min_size=20.0, motion=1)
START = (300.0, 400.0)


def walker(frames, vx, vy):
    """The true poses [frames, J, 3] of the figure translating by (vx, vy) pixels a frame from START; score 0.75 everywhere."""
    out = np.zeros((frames, J, 3), np.float64)
    for f in range(frames):
        out[f, :, 0] = FIGURE[:, 0] + (START[0] + vx * f)
        out[f, :, 1] = FIGURE[:, 1] + (START[1] + vy * f)
        out[f, :, 2] = 0.75
    return out


def noisy(truth, seed, sd=1.5):
    """truth + N(0, sd) per joint, coordinate and frame."""
    rs = np.random.RandomState(seed)
    out = truth.copy()
    out[:, :, :2] += rs.randn(*truth[:, :, :2].shape) * sd
    return out


def ratios(truth, raw, smooth, after=40):
    """-> (RMS second difference of smooth / of raw, mean |smooth - truth| / mean |raw - truth|), both over the frames from `after`."""
    t, r, s = truth[after:, :, :2], raw[after:, :, :2], smooth[after:, :, :2]

    def rms2(a):
        d = a[2:] - 2.0 * a[1:-1] + a[:-2]
        return float(np.sqrt((d * d).mean()))

    return rms2(s) / rms2(r), float(np.abs(s - t).mean()) / float(np.abs(r - t).mean())


SPEEDS = (0.0, 3.0, 12.0)  # pixels a frame along x; half of it along y
