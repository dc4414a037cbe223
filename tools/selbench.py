"""Selective reads against what a caller does without them: a full decode
(and, for Int32, values[mask] in torch).

Columns: C2-shaped Int32 (8192-row pages, adaptive ratio 1.2), C3-shaped
nullable Utf8 (LZ4 pages) and C4-shaped List<Int32> (nullable lists of
nullable items, lengths 0..2, adaptive ratio 1.2).  Selections: all rows, one 1 % range not aligned
to pages, ten 0.1 % ranges, Bernoulli 10 % and 0.1 %.  Per (column,
selection) the variants are timed with HIP events after a warm-up,
alternating inside one loop, medians reported; the plan (resolve + page
tables, with its readback) is timed on the host.  The file leg reads the
columns from a strawboat file: whole-chunk upload + full decode against
StrawboatFile.read_selected / read_selected_list, wall clock, with the bytes
uploaded; for the List column the share of page_rows (one 4-byte read per
page before anything is uploaded) is reported on its own.

python tools/selbench.py [--int-rows N] [--utf8-rows N] [--list-rows N] [--columns a,b] [--reps K] [--out FILE]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def selections(n, seed=17):
    rng = np.random.default_rng(seed)
    out = {"all": [(0, n)]}
    a = int(0.37 * n) + 123
    out["range_1pct"] = [(a, a + n // 100)]
    w = n // 1000
    out["ten_0.1pct"] = [(int((0.05 + 0.09 * i) * n) + 7 * i + 1, int((0.05 + 0.09 * i) * n) + 7 * i + 1 + w) for i in range(10)]
    out["bernoulli_10pct"] = rng.random(n) < 0.10
    out["bernoulli_0.1pct"] = rng.random(n) < 0.001
    return out


def timed(torch, variants, reps, warmup=3):
    """variants: name -> callable (launches on the current stream) -> median ms per variant."""
    for _ in range(warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    evs = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            evs[k].append((a, b))
    torch.cuda.synchronize()
    return {k: float(np.median([a.elapsed_time(b) for a, b in v])) for k, v in evs.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--int-rows", type=int, default=20 * 1024 * 1024)
    ap.add_argument("--utf8-rows", type=int, default=5_000_000)
    ap.add_argument("--list-rows", type=int, default=5_000_000)
    ap.add_argument("--columns", default="c2_int32,c3_utf8,c4_list", help="comma-separated subset of the columns")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "select_bench.json"))
    args = ap.parse_args()

    import torch

    import bench
    import pa_amd

    ctx = pa_amd.default_context(0)
    rng = np.random.default_rng(77)
    want = args.columns.split(",")
    cols = []
    if "c2_int32" in want:
        x = bench.gen_c2(args.int_rows, 3, "mix")
        ichunk, imetas = pa_amd.encode_column(x, None, False, pa_amd.WriteOptions(default_compress_ratio=1.2,
                                                                                  max_page_size=8192, seed=3))
        cols.append(dict(name="c2_int32", chunk=ichunk, metas=imetas, rows=args.int_rows, kind="flat"))
    if "c3_utf8" in want:
        svals, soffs = bench.decimal_strings(rng.integers(0, 10**6, args.utf8_rows))
        svalid = rng.random(args.utf8_rows) >= 0.1
        schunk, smetas = pa_amd.encode_binary_column(svals, soffs, svalid, True,
                                                     pa_amd.WriteOptions(default_compression=1, max_page_size=8192, seed=1))
        cols.append(dict(name="c3_utf8", chunk=schunk, metas=smetas, rows=args.utf8_rows, kind="binary"))
    if "c4_list" in want:  # bench.WorkloadC4's shape
        lens = rng.integers(0, 3, args.list_rows)
        lvalid = rng.random(args.list_rows) >= 0.1
        lens[~lvalid] = 0
        loffs = np.zeros(args.list_rows + 1, np.int64)
        np.cumsum(lens, out=loffs[1:])
        child = rng.integers(0, 1 << 16, int(loffs[-1])).astype(np.int32)
        cvalid = rng.random(int(loffs[-1])) >= 0.2
        lchunk, lmetas = pa_amd.encode_list_column(loffs, child, lvalid, cvalid, True, True,
                                                   pa_amd.WriteOptions(default_compress_ratio=1.2, max_page_size=8192,
                                                                       seed=4))
        cols.append(dict(name="c4_list", chunk=lchunk, metas=lmetas, rows=args.list_rows, kind="list",
                         leaves=int(loffs[-1])))
    records = []
    for col in cols:
        n = col["rows"]
        dchunk = torch.from_numpy(np.frombuffer(col["chunk"], np.uint8).copy()).cuda()
        if col["kind"] == "binary":
            full = pa_amd.BinaryColumnDecoder(dchunk, col["metas"], pa_amd.UTF8, True, ctx)
        elif col["kind"] == "list":
            full = pa_amd.ListColumnDecoder(dchunk, col["metas"], np.int32, True, True, ctx)
        else:
            full = pa_amd.ColumnDecoder(dchunk, col["metas"], np.int32, False, ctx)
        fout = full.alloc_outputs()
        full.decode(*fout)
        for sname, what in selections(n).items():
            if isinstance(what, list):
                sel = pa_amd.Selection(ranges=what, n_rows=n, device="cuda")
                mask = torch.zeros(n, dtype=torch.bool, device="cuda")
                for a, b in what:
                    mask[a:b] = True
            else:
                mask = torch.from_numpy(what).cuda()
                sel = pa_amd.Selection(mask=mask)
            plan_ms = []
            dec = None
            for _ in range(3):
                if dec is not None:
                    dec.close()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if col["kind"] == "binary":
                    dec = pa_amd.BinaryColumnDecoder.select(dchunk, col["metas"], pa_amd.UTF8, True, sel, ctx)
                elif col["kind"] == "list":  # (the page rows are read from the chunk inside the plan time)
                    dec = pa_amd.ListColumnDecoder.select(dchunk, col["metas"], np.int32, True, True, sel, ctx)
                else:
                    dec = pa_amd.ColumnDecoder.select(dchunk, col["metas"], np.int32, False, sel, ctx)
                plan_ms.append((time.perf_counter() - t0) * 1e3)
            sout = dec.alloc_outputs()
            got = dec.decode(*sout)
            variants = {"full_decode": lambda: full.decode_async(*fout), "select": lambda: dec.decode_async(*sout)}
            ok = None
            if col["kind"] == "flat":
                variants["full_decode+mask"] = lambda: (full.decode_async(*fout), fout[0][:n][mask])
                ok = bool(torch.equal(got[0], fout[0][:n][mask]))
            ms = timed(torch, variants, args.reps)
            direct, compacted, scratch = dec.stats()
            rec = dict(column=col["name"], rows=n, pages=len(col["metas"]), chunk_bytes=len(col["chunk"]),
                       selection=sname, selected_rows=dec.num_rows, touched_pages=dec.num_pages, pages_direct=direct,
                       pages_compacted=compacted, scratch_bytes=scratch, plan_ms=float(np.median(plan_ms)), ms=ms,
                       matches_mask=ok)
            if col["kind"] == "list":
                rec.update(leaves=col["leaves"], leaf_bound=dec.leaf_bound, selected_leaves=dec.written_leaves())
            records.append(rec)
            print(json.dumps(rec), flush=True)
            dec.close()
        full.close()
        del dchunk, fout

    # the file leg: whole-chunk upload + full decode against read_selected
    try:
        import pyarrow as pa
    except ImportError:
        pa = None
    if pa is not None:
        fields = {"c2_int32": pa.field("a", pa.int32(), False), "c3_utf8": pa.field("s", pa.utf8(), True),
                  "c4_list": pa.field("l", pa.list_(pa.field("item", pa.int32(), True)), True)}
        schema = pa.schema([fields[c["name"]] for c in cols])
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "sel.sb")
            with open(path, "wb") as fh:
                fh.write(pa_amd.assemble_file([(c["chunk"], c["metas"]) for c in cols], schema.serialize().to_pybytes()[8:]))
            with pa_amd.StrawboatFile(path) as f:
                for c, col in enumerate(cols):
                    n = col["rows"]
                    for sname, what in selections(n).items():
                        sel = pa_amd.Selection(ranges=what, n_rows=n, device="cuda") if isinstance(what, list) \
                            else pa_amd.Selection(mask=torch.from_numpy(what).cuda())
                        t = {"file_full": [], "file_select": []}
                        for _ in range(5):
                            torch.cuda.synchronize()
                            t0 = time.perf_counter()
                            dec = f.decoder(c, ctx)
                            dec.decode()
                            torch.cuda.synchronize()
                            t["file_full"].append((time.perf_counter() - t0) * 1e3)
                            dec.close()
                            t0 = time.perf_counter()
                            if col["kind"] == "list":
                                f.read_selected_list(c, sel, ctx)
                            else:
                                f.read_selected(c, sel, ctx)
                            torch.cuda.synchronize()
                            t["file_select"].append((time.perf_counter() - t0) * 1e3)
                            if col["kind"] == "list":  # its fixed cost per page, on its own
                                t0 = time.perf_counter()
                                f.page_rows(c)
                                t.setdefault("page_rows", []).append((time.perf_counter() - t0) * 1e3)
                        rec = dict(column=col["name"], selection=sname, leg="file", chunk_bytes=len(col["chunk"]),
                                   uploaded_bytes=f.last_uploaded_bytes,
                                   wall_ms={k: float(np.median(v)) for k, v in t.items()})
                        records.append(rec)
                        print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(dict(tool="tools/selbench.py", reps=args.reps, records=records), fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
