"""Nested device encode against the host writer on one shape:
struct<name: LargeUtf8, age: List<Int32>> (io.rs's test_struct_list), 8192-row
pages, at ratio 1.2 and under default LZ4.

python tools/nestencbench.py [rows] [repeats]

Device: pa_amd.encode_field_device on arrays in HBM, warm-up then `repeats`
runs timed with a host clock around the synchronizing call.  Host:
pa_amd.encode_field on 16 threads, in the same run.  `--once` encodes once
per option set on the device and exits (for a kernel trace)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build(rows, rng):
    import bench
    import pa_amd

    fld = pa_amd.Field.struct([
        pa_amd.Field.leaf(pa_amd.LARGE_UTF8, True, "name"),
        pa_amd.Field.list(pa_amd.Field.leaf(np.int32, True, "item"), True, name="age")], False)
    data, offs = bench.decimal_strings(rng.integers(0, rows, rows))
    name = pa_amd.HostArray("leaf", rows, rng.random(rows) > 0.2, values=(offs, data))
    lv = rng.random(rows) > 0.1
    lens = np.where(lv, rng.integers(0, 3, rows), 0)
    lo = np.zeros(rows + 1, np.int64)
    np.cumsum(lens, out=lo[1:])
    m = int(lo[-1])
    item = pa_amd.HostArray("leaf", m, rng.random(m) > 0.2, values=rng.integers(0, max(m, 1), m).astype(np.int32))
    age = pa_amd.HostArray("list", rows, lv, lo, [item])
    return fld, pa_amd.HostArray("struct", rows, None, children=[name, age])


def main():
    import torch

    import pa_amd

    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    once = "--once" in sys.argv
    rows = int(args[0]) if args else 10_000_000
    reps = int(args[1]) if len(args) > 1 else 20
    fld, host = build(rows, np.random.default_rng(7))
    dev = pa_amd.device_array(host, 0)
    ctx = pa_amd.default_context(0)
    in_bytes = len(host.children[0].values[1]) + 8 * (rows + 1) * 2 + 4 * host.children[1].children[0].length
    for label, o in (("ratio1.2", pa_amd.WriteOptions(default_compress_ratio=1.2, max_page_size=8192, seed=1)),
                     ("lz4", pa_amd.WriteOptions(default_compression=1, max_page_size=8192, seed=1))):
        d = pa_amd.encode_field_device(fld, dev, o, ctx)  # warm-up: grows the context scratch
        torch.cuda.synchronize()
        if once:
            continue
        t0 = time.perf_counter()
        for _ in range(reps):
            d = pa_amd.encode_field_device(fld, dev, o, ctx)  # (synchronizes the stream)
        dt = (time.perf_counter() - t0) / reps
        t0 = time.perf_counter()
        h = pa_amd.encode_field(fld, host, o, n_threads=16)
        ht = time.perf_counter() - t0
        same = all(dc.cpu().numpy().tobytes() == hc for (dc, _), (hc, _) in zip(d, h))
        print(f"{label}: rows {rows} device {dt * 1e3:.2f} ms ({in_bytes / dt / 1e9:.2f} GB/s in) host16 {ht * 1e3:.2f} ms "
              f"host/device {ht / dt:.2f}x chunk bytes {sum(len(c) for c, _ in h)} byte-identical {same}", flush=True)


if __name__ == "__main__":
    main()
