"""Hand-built LZ4 and Snappy streams on the device (tests/lzgen.py builds
them, states which are valid and wraps them into pages; tests/
test_lz_model_cpu.py holds those statements to liblz4, the oracle's Snappy
decoder and Google's).

Valid streams must decode to the plain replay of their sequence list at each
place the device routes a stream differently: a fixed-width leaf (k_inflate:
lz4_inflate / snappy_wave<true>), the exceptions of a Freq page and the
index stream of a Dict page (the deferred pass: expand_to_lds, lz4_wave<false>
/ snappy_wave<false>), a Dict page sized so that the deferred pass queues
its index stream for expansion into HBM (expand_to_hbm), and the offsets and
values streams of Binary / Utf8 / LargeUtf8 Basic pages (k_inflate, the
offsets rebased on the way or through scratch).  A Dict index
stream has to hold indices, so it takes the word-safe case set (offsets that
are multiples of 4); the Freq exceptions are plain bytes and take every case.
Every column is one decode call over hundreds of pages of odd sizes, so the
pages' output bases and the streams' starts take every alignment.

Streams the model rejects must be refused with E_CODEC at their page, the
others must decode to the model's bytes: the device rejects exactly what
LZ4_decompress_safe (and, for Snappy, the oracle's decoder) rejects."""
import ctypes
import time

import numpy as np
import pytest

from oracle import oracle as O
from tests import lzgen as G
from tests.colgen import gen_values

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TAIL = 64
CODECS = [O.LZ4, O.SNAPPY]
IDS = ["lz4", "snappy"]


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pa_amd

    return pa_amd.default_context(0)


def _guarded(nbytes):
    """A device buffer of nbytes with a 0xA5 tail behind it -> (whole, view of the first nbytes)."""
    whole = torch.full((nbytes + TAIL,), 0xA5, dtype=torch.uint8, device="cuda")
    return whole, whole[:nbytes]


def _tail_ok(whole):
    return bool((whole[-TAIL:] == 0xA5).all())


def decode(ctx, pages, nullable):
    """One decode call over `pages` [(bytes, rows)] of an Int8 column ->
    (status, bad page, values as uint8, validity bools | None)."""
    import pa_amd
    from pa_amd import _native as N

    chunk = b"".join(p for p, _ in pages)
    dec = pa_amd.ColumnDecoder(chunk, [pa_amd.PageMeta(len(p), n) for p, n in pages], np.int8, nullable, ctx)
    try:
        rows = dec.num_rows
        vw, v = _guarded(max(rows, 1))
        words = 4 * max((rows + 31) // 32, 1)
        mw, m = _guarded(words) if nullable else (None, None)
        if nullable:
            m.zero_()
        dec.decode_async(v, m)
        bad = ctypes.c_int64(-1)
        st = N.lib().sb_plan_status(ctx._h, dec._h, ctypes.byref(bad))
        assert _tail_ok(vw), "the guard behind the values was written"
        assert mw is None or _tail_ok(mw), "the guard behind the validity was written"
        vals = v.cpu().numpy()[:rows]
        bits = np.unpackbits(m.cpu().numpy(), bitorder="little")[:rows].astype(bool) if nullable else None
        return st, bad.value, vals, bits
    finally:
        dec.close()


def _cases(codec):
    return G.lz4_valid_cases() if codec == O.LZ4 else G.snappy_valid_cases()


def _check_column(ctx, items, nullable, what):
    """items: [(name, page, rows, expected uint8 array, validity | None)]."""
    st, bad, vals, bits = decode(ctx, [(p, n) for _, p, n, _, _ in items], nullable)
    assert st == 0, f"{what}: status {st} at page {bad} ({items[bad][0] if bad >= 0 else '-'})"
    row = 0
    wrong = []
    for name, _, n, exp, val in items:
        got = vals[row:row + n]
        if got.tobytes() != exp.tobytes():
            d = np.flatnonzero(got != exp)
            wrong.append(f"{name}: {len(d)} of {n} bytes differ, first at {d[0]} (row {row + d[0]})")
        elif nullable and not (bits[row:row + n] == val).all():
            wrong.append(f"{name}: validity differs")
        row += n
    assert not wrong, f"{what}: {len(wrong)} of {len(items)} pages wrong: {wrong[:6]}"


def _u8(b):
    return np.frombuffer(b, np.uint8)


@pytest.mark.parametrize("nullable", [False, True], ids=["req", "null"])
@pytest.mark.parametrize("codec", CODECS, ids=IDS)
def test_valid_streams_as_leaf_pages(ctx, codec, nullable):
    """P1: every valid stream as the values of an Int8 page, twice (the second
    time in another order, with the header's unread usize field off by one)."""
    t0 = time.perf_counter()
    cases = _cases(codec)
    order = list(range(len(cases))) + list(np.random.default_rng(5).permutation(len(cases)))
    items = []
    for j, i in enumerate(order):
        k = cases[i]
        val = G.validity_bits(k.olen, j) if nullable else None
        page, n = G.leaf_page(k, val, usize=None if j < len(cases) else k.olen + j % 3 - 1)
        items.append((k.name, page, n, _u8(k.out), val))
    starts = np.cumsum([0] + [n for _, _, n, _, _ in items])[:-1]
    assert len(set(int(s) % 16 for s in starts)) == 16  # every output alignment
    _check_column(ctx, items, nullable, "leaf pages")
    print(f"leaf {IDS[CODECS.index(codec)]} nullable={nullable}: {len(items)} pages, {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("nullable", [False, True], ids=["req", "null"])
@pytest.mark.parametrize("codec", CODECS, ids=IDS)
def test_valid_streams_as_freq_exceptions(ctx, codec, nullable):
    """P2: every valid stream as a Freq page's exceptions stream, expanded in
    LDS by the deferred pass."""
    t0 = time.perf_counter()
    items = []
    for j, k in enumerate(_cases(codec)):
        n = G.freq_rows(k.olen)[0]
        val = G.validity_bits(n, j) if nullable else None
        page, n = G.freq_page(k, val)
        items.append((k.name, page, n, G.freq_expected(k, k.out), val))
    _check_column(ctx, items, nullable, "Freq exceptions")
    print(f"freq {IDS[CODECS.index(codec)]} nullable={nullable}: {len(items)} pages, {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("spill", [False, True], ids=["lds", "hbm"])
@pytest.mark.parametrize("codec", CODECS, ids=IDS)
def test_valid_streams_as_dict_indices(ctx, codec, spill):
    """P2 / P3: the word-safe streams as a Dict page's index stream: in LDS,
    and (the dictionary enlarged until page and indices no longer fit the
    deferred pass's LDS together) expanded into HBM."""
    t0 = time.perf_counter()
    items = []
    for j, k in enumerate(G.word_cases(codec)):
        nullable_rows = k.olen // 4
        val = G.validity_bits(nullable_rows, j)
        page, n = G.dict_page(k, val, G.spill_entries(k, val) if spill else G.DICT_K)
        items.append((k.name, page, n, G.dict_expected(k.out), val))
    _check_column(ctx, items, True, "Dict indices")
    print(f"dict {IDS[CODECS.index(codec)]} spill={spill}: {len(items)} pages, {time.perf_counter() - t0:.2f} s")


def test_pyarrow_snappy_streams(ctx):
    """Streams of Google's compressor (copy-1 heavy, unlike the oracle's) as
    leaf pages and as Freq exceptions."""
    pa = pytest.importorskip("pyarrow")
    if not pa.Codec.is_available("snappy"):
        pytest.skip("pyarrow without snappy")
    t0 = time.perf_counter()
    rng = np.random.default_rng(21)
    codec = pa.Codec("snappy")
    cases = []
    census = {}
    for kind in ("index", "full", "sorted", "one", "runs", "short_runs", "freq", "bits3"):
        for dt, n in ((np.int32, 9001), (np.int64, 2500), (np.uint8, 7777)):
            raw = gen_values(kind, n, dt, rng, uniq=300).tobytes()
            block = codec.compress(raw).to_pybytes()
            assert G.snappy_model(block, len(raw)) == raw
            for key, c in G.snappy_census(block).items():
                census[key] = census.get(key, 0) + c
            cases.append(G.Case(f"{kind}/{np.dtype(dt).name}", O.SNAPPY, block, len(raw), raw))
    assert census.get("copy1", 0) > 100, census
    leaf, freq = [], []
    for k in cases:
        page, n = G.leaf_page(k)
        leaf.append((k.name, page, n, _u8(k.out), None))
        page, n = G.freq_page(k)
        freq.append((k.name, page, n, G.freq_expected(k, k.out), None))
    _check_column(ctx, leaf, False, "pyarrow leaf pages")
    _check_column(ctx, freq, False, "pyarrow Freq exceptions")
    print(f"pyarrow snappy: {len(cases)} streams, {census}, {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("kind", ["binary", "utf8-null", "large_utf8"])
@pytest.mark.parametrize("codec", CODECS, ids=IDS)
def test_valid_streams_as_binary_pages(ctx, codec, kind):
    """P4: Basic pages whose offsets stream and values stream are both
    hand-built.  Every page but the first rebases its offsets onto the values
    before it (Utf8: in place while the stream is expanded, far reads
    included; LargeUtf8: through scratch).  Binary takes every other class A
    stream as values, the Utf8 kinds the ASCII set."""
    import pa_amd
    from pa_amd import binary as B

    t0 = time.perf_counter()
    phys, ow, nullable = {"binary": (B.BINARY, 4, False), "utf8-null": (B.UTF8, 4, True),
                          "large_utf8": (B.LARGE_UTF8, 8, False)}[kind]
    vals_cases = [k for k in _cases(codec) if "big" not in k.tags][::2] if kind == "binary" else G.ascii_cases(codec)
    pages, offs, vals, valid = G.binary_column(codec, ow, vals_cases, nullable)
    chunk = b"".join(p for p, _ in pages)
    dec = pa_amd.BinaryColumnDecoder(chunk, [pa_amd.PageMeta(len(p), n) for p, n in pages], phys, nullable, ctx)
    try:
        rows = dec.num_rows
        assert rows == len(offs) - 1 and dec.values_bytes == len(vals)
        ow_, o = _guarded((rows + 1) * ow)
        vw, v = _guarded(max(len(vals), 16))
        mw, m = _guarded(4 * max((rows + 31) // 32, 1)) if nullable else (None, None)
        o.zero_()
        if nullable:
            m.zero_()
        dec.decode(o.view(torch.int32 if ow == 4 else torch.int64), v, m)
        torch.cuda.synchronize()
        assert _tail_ok(ow_) and _tail_ok(vw) and (mw is None or _tail_ok(mw)), "a guard was written"
        go = o.cpu().numpy().view("<i4" if ow == 4 else "<i8").astype(np.int64)
        bad = np.flatnonzero(go != offs)
        assert not len(bad), f"{len(bad)} offsets differ, first at row {bad[0]}: {go[bad[0]]} != {offs[bad[0]]}"
        gv = v.cpu().numpy()[:len(vals)]
        bad = np.flatnonzero(gv != _u8(vals))
        assert not len(bad), f"{len(bad)} value bytes differ, first at {bad[0]}"
        if nullable:
            gm = np.unpackbits(m.cpu().numpy(), bitorder="little")[:rows].astype(bool)
            assert (gm == valid).all(), "validity differs"
    finally:
        dec.close()
    print(f"binary {IDS[CODECS.index(codec)]} {kind}: {len(pages)} pages, {rows} rows, {time.perf_counter() - t0:.2f} s")


def _good(codec):
    return next(k for k in _cases(codec) if k.name == ("tail9" if codec == O.LZ4 else "lit_nb0_59"))


def _verdicts(ctx, cases, wrap, expected):
    """Each stream as page 1 of three (its neighbours valid): refused with
    E_CODEC at page 1 exactly when the model rejects it, else the model's bytes."""
    from pa_amd import _native as N

    good = _good(cases[0].codec)
    first, last = wrap(good), wrap(good)
    seen = {"ok": 0, "err": 0}
    wrong = []
    for k in cases:
        m = G.model(k)
        st, bad, vals, _ = decode(ctx, [first, wrap(k), last], False)
        if m is None:
            seen["err"] += 1
            if st == 0:
                wrong.append(f"{k.name}: the model rejects the stream, the device decodes it")
            elif st != N.E_CODEC or bad != 1:
                wrong.append(f"{k.name}: status {st} at page {bad}, expected {N.E_CODEC} at page 1")
        else:
            seen["ok"] += 1
            if st != 0:
                wrong.append(f"{k.name}: the model decodes the stream, the device reports status {st} at page {bad}")
            elif vals[first[1]:first[1] + wrap(k)[1]].tobytes() != expected(k, m).tobytes():
                wrong.append(f"{k.name}: bytes differ")
    assert not wrong, f"{len(wrong)} of {len(cases)} verdicts wrong: {wrong[:12]}"
    return seen


PLACES = {
    "leaf": (lambda k: G.leaf_page(k), lambda k, m: _u8(m)),
    "freq": (lambda k: G.freq_page(k), lambda k, m: G.freq_expected(k, m)),
}


@pytest.mark.parametrize("place", list(PLACES))
@pytest.mark.parametrize("codec", CODECS, ids=IDS)
def test_edited_streams_match_model(ctx, codec, place):
    """Class B: streams with one rule broken each (LZ4: the end-of-block
    rules, offsets past the start and of 0, cuts, trailing bytes, the size off
    by one)."""
    t0 = time.perf_counter()
    cases = G.lz4_edit_cases() + G.lz4_offset0_cases() if codec == O.LZ4 else G.snappy_edit_cases()
    seen = _verdicts(ctx, cases, *PLACES[place])
    assert seen["err"] and (seen["ok"] or codec == O.SNAPPY)
    print(f"edits {IDS[CODECS.index(codec)]} {place}: {seen}, {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("place", list(PLACES))
@pytest.mark.parametrize("codec", CODECS, ids=IDS)
def test_flipped_streams_match_model(ctx, codec, place):
    """A fixed seeded set of 300 streams with 1-3 flipped bits."""
    t0 = time.perf_counter()
    seen = _verdicts(ctx, G.flip_cases(codec), *PLACES[place])
    assert seen["ok"] and seen["err"]
    print(f"flips {IDS[CODECS.index(codec)]} {place}: {seen}, {time.perf_counter() - t0:.2f} s")
