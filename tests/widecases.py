"""The option sets, data shapes and page sizes the wide-integer tests share."""
from __future__ import annotations

import numpy as np

from oracle import oracle as O

# every option set the suite's integer columns are written with
OPTS = {
    "default": dict(),
    "ratio1.2": dict(ratio=1.2),
    "ratio2": dict(ratio=2.0),
    "lz4": dict(default_codec=O.LZ4),
    "zstd": dict(default_codec=O.ZSTD),
    "snappy": dict(default_codec=O.SNAPPY),
    "ratio1.2_lz4": dict(ratio=1.2, default_codec=O.LZ4),
    "ratio2_zstd": dict(ratio=2.0, default_codec=O.ZSTD),
    "forced_dict": dict(ratio=2.0, forced=O.DICT),
    "forced_dict_lz4": dict(ratio=2.0, forced=O.DICT, default_codec=O.LZ4),
    "forced_rle": dict(forced=O.RLE),
    "forced_freq": dict(ratio=2.0, forced=O.FREQ),
    "forced_freq_r1": dict(ratio=1.0, forced=O.FREQ),
    "forced_bp": dict(ratio=0.0001, forced=O.BITPACKING),
    "forced_bp_r2": dict(ratio=2.0, forced=O.BITPACKING),
    "basic_only": dict(ratio=1.0, forbidden=(O.DICT, O.FREQ, O.RLE, O.ONE_VALUE)),
    "no_freq": dict(ratio=1.2, forbidden=(O.FREQ,)),
    "seed3": dict(ratio=1.2, seed=3),
}
SIZES = (640, 641, 650)  # either side of the sampler's threshold (n / 10 <= 64 encodes the whole page)
SHAPES = ("constant", "few", "dominant", "runs", "random", "all_null", "mostly_null")


def shape(kind: str, n: int, W: int, rng: np.random.Generator):
    """-> (values as Python ints over the full width, validity).  Negatives,
    the +-2^(8W-1) edges, 0 and -1, and values that differ only in the top or
    only in the bottom limb."""
    bits = 8 * W
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    top_only = [(k << (bits - 64)) + 12345 for k in (-3, -1, 1, 2)]     # differ in the top limb alone
    bottom_only = [(5 << (bits - 64)) + k for k in (0, 1, 2, (1 << 63))]  # differ in the bottom limb alone
    pool = [lo, hi, 0, -1, 1, lo + 1, hi - 1] + top_only + bottom_only

    def rnd():
        return int.from_bytes(rng.bytes(W), "little", signed=True)

    valid = rng.random(n) > 0.2
    if kind == "constant":
        vals = [pool[7]] * n
    elif kind == "few":
        vals = [pool[int(i)] for i in rng.integers(0, len(pool), n)]
    elif kind == "dominant":  # one value on ~95 % of the rows, a large maximum
        vals = [top_only[2] if rng.random() < 0.95 else rnd() for _ in range(n)]
    elif kind == "runs":
        vals = []
        while len(vals) < n:
            vals += [pool[int(rng.integers(0, len(pool)))] if rng.random() < 0.5 else rnd()] * int(rng.integers(1, 40))
        vals = vals[:n]
    elif kind == "random":
        vals = [rnd() for _ in range(n)]
    elif kind == "all_null":
        vals, valid = [rnd() for _ in range(n)], np.zeros(n, bool)
    elif kind == "mostly_null":
        vals, valid = [rnd() for _ in range(n)], rng.random(n) > 0.93
    else:
        raise ValueError(kind)
    return vals, valid
