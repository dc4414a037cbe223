"""Int128 / Int256 columns on the device against tests/widegen.py's reader:
bit-exact values (the bytes under null slots included) and validity, for
W in {16, 32}, nullable or not.  Pages come from the model's builders, so
every codec and cascade is met whether a writer would choose it or not."""
import ctypes

import numpy as np
import pytest

from oracle import oracle as O
from tests import widegen as G
from tests.widecases import shape

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SIZES = (1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 1000, 4095)  # 4095: past the 48 KiB stage at both widths
WIDTHS = (16, 32)


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pa_amd

    return pa_amd.default_context(0)


_VALUES = {}


def values(kind, n, W):
    """Seeded values of a shape, built once per (kind, n, W) and left unchanged."""
    key = (kind, n, W)
    if key not in _VALUES:
        _VALUES[key] = shape(kind, n, W, np.random.default_rng(n * 64 + W + len(kind)))[0]
    return _VALUES[key]


def valid_bits(n, seed=1):
    return np.random.default_rng(seed + n).random(n) > 0.25


def build(codec, vals, W):
    """The value stream of `vals` under the named codec / cascade."""
    n = len(vals)
    if codec in ("none", "lz4", "zstd", "snappy"):
        return G.basic_stream({"none": G.NONE, "lz4": G.LZ4, "zstd": G.ZSTD, "snappy": G.SNAPPY}[codec], vals, W)
    if codec == "one":
        return G.one_value_stream(vals[0], n, W)
    if codec == "rle":
        return G.rle_stream(G.runs_of(vals), n, W)
    if codec == "dict":
        idx, sets = G.dictionary(vals)
        return G.dict_stream(G.index_stream(G.NONE, idx), sets, n, W)
    top = max(set(vals), key=vals.count)
    pos, exc = G.freq_split(vals, top)
    if codec == "freq":
        return G.freq_stream(G.to_bytes(top, W), pos, G.none_stream(exc, W), n, W)
    if codec == "freq_dict":  # Dict under Freq: the exceptions are a Dict stream
        idx, sets = G.dictionary(exc)
        return G.freq_stream(G.to_bytes(top, W), pos, G.dict_stream(G.index_stream(G.NONE, idx), sets, len(exc), W), n, W)
    if codec == "dict_freq":  # Freq under Dict's index stream
        idx, sets = G.dictionary(vals)
        ti = max(set(idx), key=idx.count)
        ipos, iexc = G.freq_split(idx, ti)
        return G.dict_stream(G.freq_stream(G.u32(ti), ipos, G.index_stream(G.NONE, iexc), n, 4), sets, n, W)
    raise ValueError(codec)


def shape_for(codec, n, W):
    if codec == "one":
        return values("constant", n, W)
    if codec in ("freq", "freq_dict", "dict_freq"):
        return values("dominant" if codec == "freq" else "few", n, W)
    return values("runs" if codec == "rle" else "few", n, W)


def decode(ctx, pages, W, nullable):
    """pages: [(bytes, rows)] -> (raw value bytes, validity bits | None) of the whole column."""
    import pa_amd

    chunk = b"".join(p for p, _ in pages)
    metas = [pa_amd.PageMeta(len(p), n) for p, n in pages]
    dec = pa_amd.ColumnDecoder(chunk, metas, np.dtype(f"V{W}"), nullable, ctx)
    try:
        v, m = dec.decode()
        torch.cuda.synchronize()
        assert v.dtype == torch.uint8 and tuple(v.shape) == (dec.num_rows, W)
        rows = dec.num_rows
        bits = np.unpackbits(m.cpu().numpy(), bitorder="little")[:rows].astype(bool) if nullable else None
        return v.cpu().numpy().tobytes(), bits
    finally:
        dec.close()


def check_column(ctx, pages, W, nullable):
    want_raw, want_valid = G.read_column(b"".join(p for p, _ in pages), [(len(p), n) for p, n in pages], W, nullable)
    raw, bits = decode(ctx, pages, W, nullable)
    assert raw == want_raw
    if nullable:
        assert (bits == want_valid).all()


CODECS = ("none", "lz4", "zstd", "snappy", "one", "rle", "dict", "freq", "freq_dict", "dict_freq")


@pytest.mark.parametrize("nullable", [False, True], ids=["req", "null"])
@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("codec", CODECS)
def test_single_pages(ctx, codec, W, nullable):
    for n in SIZES:
        vals = shape_for(codec, n, W)
        pg = G.page(build(codec, vals, W), valid_bits(n) if nullable else None, nullable, n)
        check_column(ctx, [(pg, n)], W, nullable)


@pytest.mark.parametrize("nullable", [False, True], ids=["req", "null"])
@pytest.mark.parametrize("W", WIDTHS)
def test_dict_index_streams(ctx, W, nullable):
    """Dict's u32 index stream under each u32 codec."""
    cases = [(G.NONE, 1000), (G.RLE, 1000), (G.BITPACKING, 128), (G.BITPACKING, 256), (G.DELTA_BITPACKING, 256),
             (G.LZ4, 1000), (G.ZSTD, 1000), (G.SNAPPY, 1000)]
    for codec, n in cases:
        vals = values("few", n, W)
        if codec == G.RLE:
            vals = values("runs", n, W)
        idx, sets = G.dictionary(vals)
        if codec == G.DELTA_BITPACKING:  # (sorted indices: the packer's width is that of the raw values)
            idx = sorted(idx)
        pg = G.page(G.dict_stream(G.index_stream(codec, idx), sets, n, W), valid_bits(n) if nullable else None, nullable, n)
        check_column(ctx, [(pg, n)], W, nullable)


@pytest.mark.parametrize("nullable", [False, True], ids=["req", "null"])
@pytest.mark.parametrize("W", WIDTHS)
def test_freq_exceptions(ctx, W, nullable):
    """A 9 000-row page with ~5 000 exceptions (a roaring bitmap container,
    more than 8 192 rows; under Zstd at W = 32 the exceptions expand past the
    deferred pass's LDS and spill), and one with 10 (an array container)."""
    n = 9000
    rng = np.random.default_rng(W)
    top = -(1 << (8 * W - 3)) + 77
    for n_exc, codecs in ((5000, (G.NONE, G.LZ4, G.ZSTD, G.SNAPPY)), (10, (G.NONE, G.ZSTD))):
        pos = sorted(int(x) for x in rng.choice(n, n_exc, replace=False))
        pool = values("few", 64, W)
        exc = [pool[int(i)] + int(j) for i, j in zip(rng.integers(0, 64, n_exc), rng.integers(1, 50, n_exc))]
        for c in codecs:
            body = G.freq_stream(G.to_bytes(top, W), pos, G.basic_stream(c, exc, W), n, W)
            check_column(ctx, [(G.page(body, valid_bits(n) if nullable else None, nullable, n), n)], W, nullable)


@pytest.mark.parametrize("nullable", [False, True], ids=["req", "null"])
@pytest.mark.parametrize("W", WIDTHS)
def test_rle_past_the_fast_rows(ctx, W, nullable):
    n = 9000
    vals = values("runs", n, W)
    pg = G.page(G.rle_stream(G.runs_of(vals), n, W), valid_bits(n) if nullable else None, nullable, n)
    check_column(ctx, [(pg, n)], W, nullable)
    # zero-count runs are skipped by the reference's loop (rle.rs:115-132)
    runs = G.runs_of(values("runs", 300, W))
    runs = runs[:3] + [(0, 99)] + runs[3:]
    pg = G.page(G.rle_stream(runs, 300, W), valid_bits(300) if nullable else None, nullable, 300)
    check_column(ctx, [(pg, 300)], W, nullable)


RAGGED = ((37, "dict"), (1000, "freq"), (1, "none"), (127, "rle"), (4095, "lz4"), (128, "dict_freq"))


@pytest.mark.parametrize("order", ["forward", "reversed"])
@pytest.mark.parametrize("nullable", [False, True], ids=["req", "null"])
@pytest.mark.parametrize("W", WIDTHS)
def test_ragged_column(ctx, W, nullable, order):
    """Pages of 37, 1000, 1, 127, 4095 and 128 rows under mixed codecs: every
    page after the first starts at a validity bit offset other than 0 mod 32."""
    pages = []
    for n, codec in (RAGGED if order == "forward" else RAGGED[::-1]):
        pages.append((G.page(build(codec, shape_for(codec, n, W), W), valid_bits(n, 7) if nullable else None, nullable, n), n))
    check_column(ctx, pages, W, nullable)


@pytest.mark.parametrize("W", WIDTHS)
def test_one_shot_calls(ctx, W):
    import pa_amd
    from pa_amd import _native as N

    n = 1000
    phys = {16: pa_amd.INT128, 32: pa_amd.INT256}[W]
    vals = values("few", n, W)
    valid = valid_bits(n)
    pg = G.page(build("dict", vals, W), valid, True, n)
    want, wv = G.read_page(pg, n, W, True)
    d = torch.from_numpy(np.frombuffer(pg, np.uint8).copy()).cuda()
    out_v = torch.empty(n * W, dtype=torch.uint8, device="cuda")
    out_m = torch.zeros(((n + 31) // 32) * 4, dtype=torch.uint8, device="cuda")
    pm = (N.PageMetaC * 1)(N.PageMetaC(len(pg), n))
    desc = N.ColumnDescC(phys, 1)
    out = N.PrimitiveOutC(out_v.data_ptr(), out_m.data_ptr())
    st = N.lib().sb_decode_column(ctx._h, ctypes.byref(desc), ctypes.c_void_p(d.data_ptr()), len(pg), pm, 1, ctypes.byref(out))
    assert st == 0, ctx.error()
    assert out_v.cpu().numpy().tobytes() == want
    assert (np.unpackbits(out_m.cpu().numpy(), bitorder="little")[:n].astype(bool) == wv).all()
    stream = build("freq", values("dominant", n, W), W)
    want, _ = G.decompress_stream(stream, 0, W, n)
    d = torch.from_numpy(np.frombuffer(stream, np.uint8).copy()).cuda()
    st = N.lib().sb_decompress_values(ctx._h, phys, ctypes.c_void_p(d.data_ptr()), len(stream), n,
                                      ctypes.c_void_p(out_v.data_ptr()))
    assert st == 0, ctx.error()
    assert out_v.cpu().numpy().tobytes() == want


def malformed(W):
    """name -> (value stream, rows): pages no writer produces; the model's reader says which the reference cannot read."""
    n = 200
    vals = values("few", n, W)
    idx, sets = G.dictionary(vals)
    k = len(sets)
    top = vals[0]
    pos, exc = G.freq_split(vals, top)
    bad_idx = list(idx)
    bad_idx[n // 2] = k
    runs = G.runs_of(values("runs", n, W))
    over = runs[:-1] + [(runs[-1][0] + 1, runs[-1][1])]
    bad_pos = pos[:-1] + [n + 3]
    out = {f"codec{c}": (G.stream(c, b"\x00" * 64 * (W // 4), 128, W), 128) for c in (14, 15, 16)}
    out["none_csize"] = (G.stream(G.NONE, G.pack(vals, W)[:-W], n, W), n)
    out["dict_index_k"] = (G.dict_stream(G.index_stream(G.NONE, bad_idx), sets, n, W), n)
    out["dict_entries_short"] = (G.dict_stream(G.index_stream(G.NONE, idx), sets, n, W, k=k, entry_bytes=G.pack(sets, W)[:-5]), n)
    out["rle_overshoot"] = (G.rle_stream(over, n, W), n)
    out["rle_short"] = (G.rle_stream(runs[:-1], n, W), n)
    # a zero-count run: the reference's loop pushes nothing and goes on (rle.rs:115-132), so the model reads it
    out["rle_zero_count"] = (G.rle_stream(runs[:2] + [(0, 5)] + runs[2:], n, W), n)
    out["roaring_row"] = (G.freq_stream(G.to_bytes(top, W), bad_pos, G.none_stream(exc, W), n, W), n)
    out["freq_top_cut"] = (G.stream(G.FREQ, G.to_bytes(top, W)[: W - 3], n, W), n)
    return out


@pytest.mark.parametrize("nullable", [False, True], ids=["req", "null"])
@pytest.mark.parametrize("W", WIDTHS)
def test_malformed_pages(ctx, W, nullable):
    """Each malformed page reports the model's class on its page while its
    neighbours decode; the device rejects exactly what the model rejects."""
    import pa_amd
    from pa_amd import _native as N

    cls = {G.E_OUT_OF_SPEC: N.E_OUT_OF_SPEC, G.E_IO: N.E_IO, G.E_CODEC: N.E_CODEC}
    good_n = 100
    good = G.page(build("dict", values("few", good_n, W), W), valid_bits(good_n) if nullable else None, nullable, good_n)
    want_good, _ = G.read_page(good, good_n, W, nullable)
    for name, (stream, n) in malformed(W).items():
        bad = G.page(stream, valid_bits(n) if nullable else None, nullable, n)
        pages = [(good, good_n), (bad, n), (good, good_n)]
        try:
            G.read_page(bad, n, W, nullable)
        except G.Malformed as err:
            e = err
        else:  # the model reads it: so does the device
            check_column(ctx, pages, W, nullable)
            continue
        chunk = b"".join(p for p, _ in pages)
        dec = pa_amd.ColumnDecoder(chunk, [pa_amd.PageMeta(len(p), r) for p, r in pages], np.dtype(f"V{W}"), nullable, ctx)
        try:
            v, _ = dec.decode_async()
            which = ctypes.c_int64(-1)
            st = N.lib().sb_plan_status(ctx._h, dec._h, ctypes.byref(which))
            assert st == cls[e.code], (name, st, e.code)
            assert which.value == 1, name
            raw = v.cpu().numpy().tobytes()
            assert raw[: good_n * W] == want_good, name
            assert raw[(good_n + n) * W:] == want_good, name
        finally:
            dec.close()


@pytest.mark.parametrize("W", WIDTHS)
def test_misaligned_values_pointer(ctx, W):
    import pa_amd
    from pa_amd import _native as N

    n = 64
    pg = build("none", values("few", n, W), W)
    dec = pa_amd.ColumnDecoder(pg, [pa_amd.PageMeta(len(pg), n)], np.dtype(f"V{W}"), False, ctx)
    try:
        buf = torch.empty(n * W + 16, dtype=torch.uint8, device="cuda")
        with pytest.raises(pa_amd.StrawboatError) as e:
            dec.decode_async(buf[4:], None)
        assert e.value.status == N.E_ARG
    finally:
        dec.close()


def test_refusals_on_the_device(ctx):
    """The plans and encoders that do not take wide types say so (E_NYI), by name."""
    import pa_amd
    from pa_amd import _native as N

    n = 64
    pg = build("none", values("few", n, 16), 16)
    metas = [pa_amd.PageMeta(len(pg), n)]
    with pytest.raises(pa_amd.StrawboatError) as e:
        pa_amd.ListColumnDecoder(pg, metas, np.dtype("V16"), False, False, ctx=ctx)
    assert e.value.status == N.E_NYI and "16" in str(e.value)
    for phys in (pa_amd.INT128, pa_amd.INT256):
        opts = pa_amd.WriteOptions().c()
        olen, npg = ctypes.c_uint64(), ctypes.c_uint64()
        st = N.lib().sb_encode_column_device(ctx._h, phys, None, None, 0, 0, ctypes.byref(opts), 0, None, 0,
                                             ctypes.byref(olen), None, 0, ctypes.byref(npg))
        assert st == N.E_NYI and str(phys) in ctx.error()


def test_file_with_decimal_columns(ctx, tmp_path):
    import decimal

    import pa_amd
    import pyarrow as pa

    n = 5000
    rng = np.random.default_rng(11)
    dctx = decimal.Context(prec=80)

    def decimals(typ, W):
        out = []
        for _ in range(n):
            mag = int.from_bytes(rng.bytes(W), "little") % (10 ** int(rng.integers(1, typ.precision + 1)))
            out.append(None if rng.random() < 0.1 else dctx.create_decimal(mag if rng.random() < 0.5 else -mag).scaleb(-typ.scale, dctx))
        return pa.array(out, type=typ)

    ints = pa.array(rng.integers(-1000, 1000, n).astype(np.int32))
    d128, d256 = decimals(pa.decimal128(38, 4), 16), decimals(pa.decimal256(76, 3), 32)
    schema = pa.schema([pa.field("i", pa.int32(), False), pa.field("d", d128.type), pa.field("e", d256.type)])
    opts = pa_amd.WriteOptions(max_page_size=1500, default_compress_ratio=1.2)
    cols = [pa_amd.encode_column(ints.to_numpy(), None, False, opts)]
    for arr, W in ((d128, 16), (d256, 32)):
        vals = np.frombuffer(arr.buffers()[1], np.uint8)[: n * W].reshape(-1, W)
        cols.append(pa_amd.encode_column(vals, np.array(arr.is_valid()), True, opts))
    p = tmp_path / "dec.sb"
    p.write_bytes(pa_amd.assemble_file(cols, schema.serialize().to_pybytes()))
    with pa_amd.StrawboatFile(str(p)) as sf:
        with pytest.raises(pa_amd.StrawboatError):  # (physical_type 0: refused unless asked for by page type)
            sf.decoder(1, ctx)
        dec = sf.decoder(1, ctx, decimal_pages=True)
        assert dec.dtype == np.dtype("V16") and dec.num_rows == n
        dec.close()
        v, m = sf.read_field(0, ctx)
        assert m is None and (v.cpu().numpy()[:n] == ints.to_numpy()).all()
        for top, arr, W in ((1, d128, 16), (2, d256, 32)):
            v, m = sf.read_field(top, ctx)
            torch.cuda.synchronize()
            back = pa.Array.from_buffers(arr.type, n, [pa.py_buffer(m.cpu().numpy().tobytes()),
                                                       pa.py_buffer(v.cpu().numpy().tobytes())])
            assert back.equals(arr)
