"""The host encoder's Int128 / Int256 pages against tests/widegen.py, byte for
byte, over the options and shapes test_wide_model_cpu.py pins to the oracle at
W = 8; the Freq edge of as_i64; a pyarrow decimal round trip; the decimal
fields of sb_leaf_info; the entry points that refuse these types."""
import decimal

import numpy as np
import pyarrow as pa
import pytest

import pa_amd
from pa_amd import _native as N
from oracle import oracle as O
from tests import widegen as G
from tests.widecases import OPTS, SHAPES, SIZES, shape

PHYS = {16: pa_amd.INT128, 32: pa_amd.INT256}


@pytest.mark.parametrize("nullable", [False, True])
@pytest.mark.parametrize("W", [16, 32])
@pytest.mark.parametrize("opt", sorted(OPTS))
def test_encoder_equals_model(opt, W, nullable):
    rng = np.random.default_rng(sum(map(ord, opt)) + W + nullable)
    for n in SIZES:
        for kind in SHAPES:
            vals, valid = shape(kind, n, W, rng)
            if not nullable:
                valid = None
            kw = OPTS[opt]
            o = O.WriteOptions.make(**kw)
            w = pa_amd.WriteOptions(default_compression=kw.get("default_codec", 0),
                                    default_compress_ratio=kw.get("ratio"),
                                    forbidden_compressions=tuple(kw.get("forbidden", ())),
                                    forced_codec=kw.get("forced", -1), seed=kw.get("seed", 42))
            want = G.write_page(vals, valid, nullable, o, W=W)
            got = pa_amd.encode_page(G.as_array(vals, W), valid, nullable, w)
            assert got == want, (opt, W, nullable, n, kind, got[:24].hex(), want[:24].hex())
            raw, mv = G.read_page(got, n, W, nullable)
            # the reader gives back every valid row (null slots hold what the codec left there)
            for i in range(n):
                if valid is None or valid[i]:
                    assert raw[i * W:(i + 1) * W] == G.to_bytes(vals[i], W), (opt, n, kind, i)
            if nullable:
                assert (mv == valid).all()


@pytest.mark.parametrize("W", [16, 32])
def test_uint8_rows_are_wide_values(W):
    vals = [(-1) ** i * (i << 70) for i in range(50)]
    a = G.as_array(vals, W)
    b = np.frombuffer(a.tobytes(), np.uint8).reshape(50, W)
    assert pa_amd.encode_page(a) == pa_amd.encode_page(b)
    ca, ma = pa_amd.encode_column(a, options=pa_amd.WriteOptions(max_page_size=16))
    cb, mb = pa_amd.encode_column(b, options=pa_amd.WriteOptions(max_page_size=16))
    assert ca == cb and ma == mb and [m.num_values for m in ma] == [16, 16, 16, 2]


@pytest.mark.parametrize("W", [16, 32])
def test_freq_edge_as_i64_truncates(W):
    """freq.rs:146 `stats.max.as_i64() >= 256` sees the low 64 bits: a page
    90 % one value with maximum 300 is Freq, with maximum 2^64 + 5 it is not."""
    n = 1000
    for mx, freq in ((300, True), ((1 << 64) + 5, False)):
        vals = [7] * n
        for i in range(0, n, 12):  # ~8 % exceptions, all distinct (no Dict) and unsorted runs of 1
            vals[i] = 8 + (i % 90)
        vals[500] = mx
        pg = pa_amd.encode_page(G.as_array(vals, W), None, False, pa_amd.WriteOptions(default_compress_ratio=1.2))
        assert pg == G.write_page(vals, None, False, O.WriteOptions.make(ratio=1.2), W=W)
        assert (pg[0] == G.FREQ) == freq, (mx, pg[0])


def test_pyarrow_decimal_roundtrip():
    rng = np.random.default_rng(9)
    ctx = decimal.Context(prec=80)
    for typ, W in ((pa.decimal128(38, 4), 16), (pa.decimal256(76, 3), 32)):
        digits = typ.precision
        src = []
        for i in range(3000):
            if rng.random() < 0.1:
                src.append(None)
            else:
                mag = int.from_bytes(rng.bytes(W), "little") % (10 ** int(rng.integers(1, digits + 1)))
                src.append(ctx.create_decimal(mag if rng.random() < 0.5 else -mag).scaleb(-typ.scale, ctx))
        arr = pa.array(src, type=typ)
        valid = np.array([x is not None for x in src])
        values = np.frombuffer(arr.buffers()[1], np.uint8)[: len(src) * W].reshape(-1, W)
        chunk, metas = pa_amd.encode_column(values, valid, True,
                                            pa_amd.WriteOptions(max_page_size=1024, default_compress_ratio=1.2))
        raw, mv = G.read_column(chunk, [(m.length, m.num_values) for m in metas], W, True)
        assert (mv == valid).all()
        back = pa.Array.from_buffers(typ, len(src), [pa.py_buffer(np.packbits(mv, bitorder="little").tobytes()),
                                                     pa.py_buffer(raw)])
        assert back.to_pylist() == arr.to_pylist()


def test_schema_decimal_fields(tmp_path):
    schema = pa.schema([pa.field("a", pa.int32()), pa.field("d", pa.decimal128(20, 4)),
                        pa.field("e", pa.decimal256(50, 3), False),
                        pa.field("l", pa.list_(pa.field("item", pa.decimal128(11, 2))))])
    leaves = pa_amd.parse_schema(schema.serialize().to_pybytes())
    assert [(l.decimal_bits, l.decimal_precision, l.decimal_scale) for l in leaves] == \
        [(0, 0, 0), (128, 20, 4), (256, 50, 3), (128, 11, 2)]
    assert [l.physical_type for l in leaves] == [N.INT32, 0, 0, 0]
    assert [l.page_type for l in leaves] == [N.INT32, pa_amd.INT128, pa_amd.INT256, pa_amd.INT128]
    assert pa_amd.Leaf("x", "Int", N.INT64, False, 0).decimal_bits == 0
    assert pa_amd.Leaf("x", "Decimal", 0, False, 0, decimal_bits=64).page_type == 0  # only 128 / 256 have pages
    # a Decimal leaf under a nest has no page path: decoder() says so before it touches a device
    p = tmp_path / "d.sb"
    p.write_bytes(pa_amd.assemble_file([(b"", [])] * 4, schema.serialize().to_pybytes()))
    with pa_amd.StrawboatFile(str(p)) as sf:
        assert sf.leaves[3].depth == 1
        with pytest.raises(pa_amd.StrawboatError) as e:
            sf.decoder(3, ctx=object(), chunk=object())
        assert e.value.status == N.E_NYI


def _status(e):
    return e.value.status


def test_refusals_without_a_device():
    v = G.as_array([1, 2, 3, 4], 16)
    offs = np.array([0, 2, 4], np.int64)
    for phys in (pa_amd.INT128, pa_amd.INT256):
        with pytest.raises(pa_amd.StrawboatError) as e:
            pa_amd.encode_list_column(offs, v if phys == pa_amd.INT128 else G.as_array([1, 2, 3, 4], 32))
        assert _status(e) == N.E_NYI
    for dt in ("V16", "V32"):
        with pytest.raises(pa_amd.StrawboatError) as e:
            pa_amd.ColumnGroupDecoder([(b"", [])], np.dtype(dt), False)
        assert _status(e) == N.E_NYI
        with pytest.raises(pa_amd.StrawboatError) as e:
            pa_amd.SelectedColumnDecoder(b"", [], np.dtype(dt), False, None)
        assert _status(e) == N.E_NYI
        with pytest.raises(pa_amd.StrawboatError) as e:
            pa_amd.encode_column_device(np.zeros(4, dt))
        assert _status(e) == N.E_NYI
    # the nested host encoder: a struct over an Int128 leaf
    with pytest.raises(pa_amd.StrawboatError) as e:
        f = pa_amd.Field("struct", False, [pa_amd.Field.leaf(np.dtype("V16"), False, "x")])
        pa_amd.encode_field(f, pa_amd.HostArray("struct", 4, children=[pa_amd.HostArray("leaf", 4, values=v)]))
    assert _status(e) == N.E_NYI
