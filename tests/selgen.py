"""Columns, selections and expected results for the selective-read tests.

Columns have ragged pages (PAGE_ROWS), so output row bases and bit offsets
take every residue mod 32.  Expected results are the oracle's full-column
decode masked with numpy on the host."""
import functools

import numpy as np

from oracle import oracle as O

PAGE_ROWS = [1, 31, 32, 33, 37, 127, 1000, 4095, 64, 8192, 5, 300]
N_ROWS = sum(PAGE_ROWS)
BOUNDS = np.concatenate([[0], np.cumsum(PAGE_ROWS)])
KINDS = ["int8", "int16", "int32", "int64", "float64", "bool", "utf8", "large_binary"]
WRITERS = ["adaptive", "lz4"]


def writer_options(writer):
    import pa_amd

    if writer == "adaptive":
        return pa_amd.WriteOptions(default_compress_ratio=1.2)
    return pa_amd.WriteOptions(default_compression=1)  # LZ4, no ratio: header-only pages


def _m(metas):
    return [(m.length, m.num_values) for m in metas]


def _strings(rng, n):
    words = [b"", b"a", b"straw", b"boat", "café".encode(), "漢字".encode(), b"0123456789" * 3]
    rows = [words[i] for i in rng.integers(0, len(words), n)]
    for i in rng.integers(0, n, n // 5):  # some distinct ones between the repeats
        rows[i] = str(int(rng.integers(0, 10**9))).encode()
    rows[BOUNDS[7] + 1234] = ("x" * 5 * 1024).encode()  # one 5 KiB row among short ones
    rows[BOUNDS[9]] = b""
    return rows


@functools.lru_cache(maxsize=None)
def column(kind, nullable, writer, page_rows=tuple(PAGE_ROWS)):
    """-> dict(chunk, metas, kind, nullable, expected...) of one column, encoded page by page."""
    import pa_amd

    n = sum(page_rows)
    bounds = np.concatenate([[0], np.cumsum(page_rows)])
    rng = np.random.default_rng(100 + 4 * KINDS.index(kind) + 2 * int(nullable) + WRITERS.index(writer))
    opts = writer_options(writer)
    valid = (rng.random(n) > 0.25) if nullable else None
    chunks, metas = [], []
    if kind in ("utf8", "large_binary"):
        phys = pa_amd.UTF8 if kind == "utf8" else pa_amd.LARGE_BINARY
        vals, offs = pa_amd.binary.strings_to_arrow(_strings(rng, n))
        for a, b in zip(bounds[:-1], bounds[1:]):
            c, m = pa_amd.encode_binary_column(vals, offs[a:b + 1], None if valid is None else valid[a:b], nullable,
                                               opts, phys)
            chunks.append(c)
            metas += m
    else:
        if kind == "bool":
            x = rng.random(n) > 0.4
        elif kind == "float64":
            x = np.round(rng.normal(0, 100, n), 2)
        else:
            dt = np.dtype(kind)
            x = (rng.integers(0, 50, n) + (np.arange(n) // 700) * 3).astype(dt)  # small domain: the cascade engages
        for a, b in zip(bounds[:-1], bounds[1:]):
            c, m = pa_amd.encode_column(x[a:b], None if valid is None else valid[a:b], nullable, opts)
            chunks.append(c)
            metas += m
    assert [m.num_values for m in metas] == list(page_rows)
    col = dict(kind=kind, nullable=nullable, chunk=b"".join(chunks), metas=metas, n=n, bounds=bounds)
    if kind in ("utf8", "large_binary"):
        col["phys"] = phys
        col["ow"] = 4 if kind == "utf8" else 8
        col["eo"], col["ev"], col["em"] = O.read_binary_column(col["chunk"], _m(metas), nullable, col["ow"])
    elif kind == "bool":
        col["ev"], col["em"] = O.read_bool_column(col["chunk"], _m(metas), nullable)
    else:
        col["ev"], col["em"] = O.read_column(col["chunk"], _m(metas), np.dtype(kind), nullable)
    return col


def bitmap(bits):
    """bool array -> the Arrow bitmap bytes the engine writes: whole 32-bit words, zero past the last row."""
    out = np.zeros(4 * ((len(bits) + 31) // 32), np.uint8)
    p = np.packbits(np.asarray(bits, bool), bitorder="little")
    out[:len(p)] = p
    return out.tobytes()


def expected(col, mask):
    """The masked oracle result as bytes: dict(values, validity[, offsets])."""
    k = int(mask.sum())
    exp = {"rows": k, "validity": bitmap(col["em"][mask]) if col["nullable"] else None}
    if "eo" in col:
        eo = col["eo"]
        starts, lens = eo[:-1][mask], np.diff(eo)[mask]
        no = np.zeros(k + 1, np.int64)
        no[1:] = np.cumsum(lens)
        src = np.frombuffer(col["ev"], np.uint8)
        idx = np.repeat(starts - no[:-1], lens) + np.arange(int(no[-1]))
        exp["offsets"] = no.astype(np.int32 if col["ow"] == 4 else np.int64).tobytes()
        exp["values"] = src[idx].tobytes()
    elif col["kind"] == "bool":
        exp["values"] = bitmap(col["ev"][mask])
    else:
        exp["values"] = col["ev"][mask].tobytes()
    return exp


def selections(n, bounds, seed=5):
    """name -> bool mask, the issue's ten selections over a column of these pages."""
    rng = np.random.default_rng(seed)
    z = lambda: np.zeros(n, bool)  # noqa: E731
    sels = {"none": z(), "all": np.ones(n, bool)}
    sels["first"] = z()
    sels["first"][0] = True
    sels["last"] = z()
    sels["last"][n - 1] = True
    edges = z()
    for b in bounds[1:-1]:  # the last row of every page and the first row of the next
        edges[b - 1] = edges[b] = True
    sels["edges"] = edges
    sels["alternate"] = np.arange(n) % 2 == 0
    sels["bernoulli_0.5"] = rng.random(n) < 0.5
    sels["bernoulli_0.02"] = rng.random(n) < 0.02
    if len(bounds) > 9:
        cut = z()  # mid-page on both sides, spans pages 6..9
        cut[bounds[6] + 333:bounds[9] + 4001] = True
        sels["range"] = cut
        holes = np.ones(n, bool)  # pages 0, 5 and the last wholly unselected; page 7 partially
        for p in (0, 5, len(bounds) - 2):
            holes[bounds[p]:bounds[p + 1]] = False
        holes[bounds[7] + 10:bounds[7] + 20] = False
        sels["holes"] = holes
    return sels


def page_counts(mask, bounds):
    return [int(mask[a:b].sum()) for a, b in zip(bounds[:-1], bounds[1:])]
