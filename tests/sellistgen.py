"""List<primitive> columns and expected results for the selective-read tests
(the selections are selgen's).

Columns lie on selgen.PAGE_ROWS: 12 ragged pages, so row bases and bit
offsets take every residue mod 32.  The rows are the smallest at which each
path of the take kernel can go wrong: lengths 0..5 with null (empty) lists,
250 consecutive empty rows across the page 5 / 6 boundary, one row of 300
leaves in page 7 (above the short-row limit: the whole-wave copy) and one of
5 000 leaves in page 9 (it spans many leaf bitmap words), 20 % null leaves.
Expected results are the oracle's full-column decode masked with numpy on
the host."""
import functools

import numpy as np

from oracle import oracle as O
from tests import selgen as S

PAGE_ROWS = S.PAGE_ROWS
N_ROWS = S.N_ROWS
BOUNDS = S.BOUNDS
LONG_ROW = (int(BOUNDS[7]) + 2000, 300)    # (row, leaves)
HUGE_ROW = (int(BOUNDS[9]) + 5000, 5000)
EMPTY_RUN = (int(BOUNDS[6]) - 125, int(BOUNDS[6]) + 125)


def arrays(dtype, seed=0):
    """-> offsets (absolute, int64), list validity, child values, child validity."""
    rng = np.random.default_rng(700 + seed)
    dtype = np.dtype(dtype)
    lens = rng.integers(0, 6, N_ROWS)
    lv = rng.random(N_ROWS) >= 0.1
    lv[[LONG_ROW[0], HUGE_ROW[0]]] = True
    lens[LONG_ROW[0]], lens[HUGE_ROW[0]] = LONG_ROW[1], HUGE_ROW[1]
    lens[EMPTY_RUN[0]:EMPTY_RUN[1]] = 0
    lens[~lv] = 0  # a null list is empty
    offs = np.zeros(N_ROWS + 1, np.int64)
    offs[1:] = np.cumsum(lens)
    n = int(offs[-1])
    if dtype.kind == "f":
        child = np.round(rng.normal(0, 100, n), 2).astype(dtype)
    else:
        child = (rng.integers(0, 50, n) + (np.arange(n) // 900) * 3).astype(dtype)  # small domain: the cascade engages
    cv = rng.random(n) >= 0.2
    return offs, lv, child, cv


def page_header(chunk, metas):
    """-> per page (start, rows, rep_len, def_len)."""
    out, pos = [], 0
    for m in metas:
        r, a, b = (int.from_bytes(chunk[pos + 4 * k:pos + 4 * k + 4], "little") for k in range(3))
        out.append((pos, r, a, b))
        pos += m.length
    return out


@functools.lru_cache(maxsize=None)
def column(dtype="int32", list_nullable=True, item_nullable=True, writer="adaptive"):
    """-> dict(chunk, metas, ...) of one List column, encoded page by page over absolute offsets."""
    import pa_amd

    dtype = np.dtype(dtype)
    offs, lv, child, cv = arrays(dtype, seed=np.dtype(dtype).itemsize + (8 if dtype.kind == "f" else 0))
    opts = S.writer_options(writer)
    chunks, metas = [], []
    for a, e in zip(BOUNDS[:-1], BOUNDS[1:]):
        c, m = pa_amd.encode_list_column(offs[a:e + 1], child, lv[a:e] if list_nullable else None,
                                         cv if item_nullable else None, list_nullable, item_nullable, opts)
        assert len(m) == 1
        chunks.append(c)
        metas += m
    chunk = b"".join(chunks)
    assert [h[1] for h in page_header(chunk, metas)] == list(PAGE_ROWS)
    return dict(dtype=dtype, ln=list_nullable, inn=item_nullable, chunk=chunk, metas=metas, n=N_ROWS, bounds=BOUNDS)


def _uleb(x):
    out = b""
    while True:
        c = x & 0x7F
        x >>= 7
        out += bytes([c | (0x80 if x else 0)])
        if not x:
            return out


def hybrid_alternating(levels, width):
    """The levels as a hybrid RLE / bit-packed stream of alternating runs: an
    RLE run of one level, then a bit-packed run of one group of 8, and so on
    (the last group padded with zeros) -> (bytes, runs)."""
    out, runs, i, n = b"", 0, 0, len(levels)
    vbytes = (width + 7) // 8
    while i < n:
        out += _uleb(1 << 1) + int(levels[i]).to_bytes(vbytes, "little")
        runs += 1
        i += 1
        if i >= n:
            break
        grp = np.zeros(8, np.uint32)
        k = min(8, n - i)
        grp[:k] = levels[i:i + k]
        bits = ((grp[:, None] >> np.arange(width)[None, :]) & 1).astype(bool).reshape(-1)
        out += _uleb((1 << 1) | 1) + np.packbits(bits, bitorder="little").tobytes()
        runs += 1
        i += k
    return out, runs


@functools.lru_cache(maxsize=None)
def walk_column():
    """The Int32 both-nullable column with every page's level streams
    rewritten as alternating RLE / bit-packed runs: far more than the 64
    runs the List kernels' run table holds, so the plan falls back to the
    general level walk.  -> the column dict + max_runs (of any one stream)."""
    import pa_amd

    col = column("int32", True, True, "adaptive")
    chunk, pages, metas, max_runs = col["chunk"], [], [], 0
    for (pos, rows, rep_len, def_len), m in zip(page_header(chunk, col["metas"]), col["metas"]):
        nlev = m.num_values
        rep = O.hybrid_decode(chunk[pos + 12:pos + 12 + rep_len], 1, nlev)
        dfs = O.hybrid_decode(chunk[pos + 12 + rep_len:pos + 12 + rep_len + def_len], 2, nlev)  # max def 3
        nrep, r1 = hybrid_alternating(rep, 1)
        ndef, r2 = hybrid_alternating(dfs, 2)
        max_runs = max(max_runs, r1, r2)
        page = (rows.to_bytes(4, "little") + len(nrep).to_bytes(4, "little") + len(ndef).to_bytes(4, "little") + nrep +
                ndef + chunk[pos + 12 + rep_len + def_len:pos + m.length])
        pages.append(page)
        metas.append(pa_amd.PageMeta(len(page), nlev))
    out = dict(col)
    out.update(chunk=b"".join(pages), metas=metas, max_runs=max_runs)
    return out


@functools.lru_cache(maxsize=None)
def _decoded(chunk, metas, dtype, ln, inn):
    return O.read_list_column(chunk, list(metas), np.dtype(dtype), ln, inn)


def decoded(col):
    """The oracle's full decode: (offsets int64, list validity | None, values, leaf validity | None)."""
    return _decoded(col["chunk"], tuple((m.length, m.num_values) for m in col["metas"]), col["dtype"].str, col["ln"],
                    col["inn"])


def expected(col, mask, large=False):
    """The masked oracle result as bytes: dict(rows, leaves, offsets, list_validity, values, leaf_validity)."""
    eo, el, ev, ef = decoded(col)
    k = int(mask.sum())
    starts, lens = eo[:-1][mask], np.diff(eo)[mask]
    no = np.zeros(k + 1, np.int64)
    no[1:] = np.cumsum(lens)
    idx = np.repeat(starts - no[:-1], lens) + np.arange(int(no[-1]))
    return {
        "rows": k,
        "leaves": int(no[-1]),
        "offsets": no.astype(np.int64 if large else np.int32).tobytes(),
        "list_validity": S.bitmap(np.asarray(el, bool)[mask]) if col["ln"] else None,
        "values": np.asarray(ev)[idx].tobytes(),
        "leaf_validity": S.bitmap(np.asarray(ef, bool)[idx]) if col["inn"] else None,
    }
