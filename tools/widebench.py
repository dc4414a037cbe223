"""Decode rate of a Decimal128 (Int128) column against an Int64 column of the
same decoded bytes, as a baseline for the W = 16 / 32 page kernels.

Columns: C2-shaped, non-nullable, 8192-row pages, values drawn from 1000
distinct ones; each written as None pages (no ratio, default codec None) and
as forced-Dict pages.  Every variant is decoded through ColumnDecoder into
preallocated outputs, timed with HIP events after a warm-up, the variants
alternating inside one loop; medians reported as GB/s of (chunk + decoded)
bytes.

python tools/widebench.py [--bytes N] [--reps K] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=64 << 20, help="decoded bytes of each column")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wide_bench.json"))
    a = ap.parse_args()
    import torch

    import pa_amd

    rng = np.random.default_rng(5)
    ctx = pa_amd.default_context(0)
    cols = {}
    for name, W in (("int64", 8), ("decimal128", 16)):
        n = a.bytes // W
        pool = rng.integers(0, 256, (1000, W), dtype=np.uint8)
        vals = pool[rng.integers(0, 1000, n)]
        vals = vals.view(np.int64).reshape(-1) if W == 8 else vals
        for codec, opts in (("none", pa_amd.WriteOptions(max_page_size=8192)),
                            ("dict", pa_amd.WriteOptions(max_page_size=8192, forced_codec=11))):
            chunk, metas = pa_amd.encode_column(vals, None, False, opts)
            dec = pa_amd.ColumnDecoder(chunk, metas, np.int64 if W == 8 else np.dtype("V16"), False, ctx)
            out, _ = dec.alloc_outputs()
            got, _ = dec.decode(out, None)
            torch.cuda.synchronize()
            assert got.cpu().numpy().tobytes() == vals.tobytes(), (name, codec)
            cols[f"{name}_{codec}"] = (dec, out, len(chunk), n * W, len(metas))
    for _ in range(5):
        for dec, out, *_ in cols.values():
            dec.decode_async(out, None)
    torch.cuda.synchronize()
    evs = {k: [] for k in cols}
    for _ in range(a.reps):
        for k, (dec, out, *_) in cols.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dec.decode_async(out, None)
            e1.record()
            evs[k].append((e0, e1))
    torch.cuda.synchronize()
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "page_rows": 8192, "columns": {}}
    for k, (dec, out, cb, db, npg) in cols.items():
        ms = float(np.median([x.elapsed_time(y) for x, y in evs[k]]))
        res["columns"][k] = {"pages": npg, "chunk_bytes": cb, "decoded_bytes": db, "median_ms": round(ms, 4),
                             "gb_per_s": round((cb + db) / ms / 1e6, 1)}
        dec.close()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
