"""The fp64 restatement of the resampler that tests/test_resample_cpu.py and tests/test_resample_gpu.py compare with: the
published formula of torchaudio's sinc_interp_hann resampler (lowpass_filter_width 6, rolloff 0.99), the dense tap table
rounded once to fp32, and the plain sum over it in fp64.  Nothing here uses audio.compact_taps."""
import functools
import math

import numpy as np

PAIRS = [(16000, 22050), (24000, 22050), (44100, 22050), (48000, 22050), (22050, 16000), (22050, 48000)]
# longest first-to-last non-zero run of a dense row, measured on the fp32-rounded table
SPANS = {(16000, 22050): 13, (24000, 22050): 14, (44100, 22050): 25, (48000, 22050): 27, (22050, 16000): 17,
         (32000, 22050): 18}


def ratio(orig, new):
    g = math.gcd(orig, new)
    o, n = orig // g, new // g
    base = min(o, n) * 0.99
    return o, n, int(math.ceil(6 * o / base)), base


@functools.lru_cache(maxsize=None)
def dense_table(orig, new):
    """K fp32 [n, 2 width + o]: t = (-i / n + (k - width) / o) base clamped to [-6, 6];
    K = sinc(pi t) cos^2(pi t / 12) base / o, sinc(0) = 1; fp64, rounded once."""
    o, n, width, base = ratio(orig, new)
    K = np.empty((n, 2 * width + o), dtype=np.float64)
    k = np.arange(2 * width + o, dtype=np.float64)
    for i in range(n):
        t = np.minimum(np.maximum((-float(i) / n + (k - width) / o) * base, -6.0), 6.0)
        x = np.pi * t
        safe = np.where(x == 0.0, 1.0, x)
        K[i] = np.where(x == 0.0, 1.0, np.sin(x) / safe) * np.cos(np.pi * t / 12.0) ** 2 * (base / o)
    K = K.astype(np.float32)
    K.setflags(write=False)
    return K


def longest_run(K):
    """the longest first-to-last non-zero stretch of a row."""
    best = 0
    for row in K:
        nz = np.flatnonzero(row)
        if nz.size:
            best = max(best, int(nz[-1] - nz[0]) + 1)
    return best


def out_length(L, orig, new):
    o, n, _, _ = ratio(orig, new)
    return -((-n * L) // o)


def noise(L, seed):
    """seeded uniform noise in [-1, 1], fp32."""
    return (np.random.default_rng(seed).random(L) * 2.0 - 1.0).astype(np.float32)


def resample_fp64(x, orig, new):
    """y[j n + i] = sum_k K[i][k] xp[j o + k] for 0 <= j n + i < ceil(n len / o), xp[m] = x[m - width] inside the row and 0
    outside; a double loop over (i, k) on the dense table, each step one fp64 product-and-add for every j at once.
    Columns whose tap is exactly zero add nothing and are skipped."""
    o, n, width, _ = ratio(orig, new)
    K = dense_table(orig, new).astype(np.float64)
    x = np.asarray(x, dtype=np.float64)
    L = x.shape[0]
    M = out_length(L, orig, new)
    J = (M + n - 1) // n
    xp = np.zeros((J - 1) * o + 2 * width + o + 1, dtype=np.float64)
    keep = min(L, xp.shape[0] - width)
    xp[width:width + keep] = x[:keep]
    y = np.zeros(J * n, dtype=np.float64)
    for i in range(n):
        acc = np.zeros(J, dtype=np.float64)
        for k in np.flatnonzero(K[i]):
            acc += K[i, k] * xp[k:k + (J - 1) * o + 1:o]
        y[i::n] = acc
    return y[:M]


def tolerance(orig, new, x):
    """(span + 1) 2^-24 max_i sum_k |K[i][k]| max|x|: the worst-case fp32 rounding of a span-term FMA chain."""
    K = dense_table(orig, new).astype(np.float64)
    return (longest_run(K) + 1) * 2.0 ** -24 * float(np.abs(K).sum(axis=1).max()) * float(np.abs(np.asarray(x)).max())
