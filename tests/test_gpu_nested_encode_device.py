"""The device writer for nested fields (pa_amd.encode_field_device ->
sb_encode_nested_column_device: k_nest_levels + the page kernels over each
page's leaf slice) against the host writer (pa_amd.encode_field) on the same
arrays: chunks and page metas equal byte for byte under None / LZ4 / Snappy
and every ratio / forced-codec option; under a Zstd default codec the same
pages and level counts, checked by decoding."""
import numpy as np
import pytest

from oracle import nest as NE
from oracle import oracle as O
from oracle.nest import A
from tests import nestgen

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

IO_CASES = ["test_struct", "test_map", "test_list_list", "test_list_struct", "test_list_map", "test_struct_list",
            "list_utf8", "list_bool", "list_list_bool"]
CODECS = {"none": O.NONE, "lz4": O.LZ4, "snappy": O.SNAPPY}
STEPS = (1, 7, 31, 32, 33, 100, 0)
SEED = 13
RLE, DICT, FREQ = 10, 11, 13


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pa_amd

    return pa_amd.default_context(0)


def metas_of(cols):
    return [[(m.length, m.num_values) for m in pm] for _, pm in cols]


def both(f, a, opts, ctx):
    """-> (host columns, device columns as host bytes)."""
    import pa_amd

    pf, ha = nestgen.pa_amd_field(f), nestgen.host_array(a)
    host = pa_amd.encode_field(pf, ha, opts)
    dev = pa_amd.encode_field_device(pf, pa_amd.device_array(ha, 0), opts, ctx)
    return host, [(c.cpu().numpy().tobytes(), pm) for c, pm in dev]


def assert_same(f, a, opts, ctx, what=""):
    host, dev = both(f, a, opts, ctx)
    assert len(host) == len(dev)
    for k, ((hc, _), (dc, _)) in enumerate(zip(host, dev)):
        assert metas_of(dev)[k] == metas_of(host)[k], (what, "leaf", k, "metas")
        assert dc == hc, (what, "leaf", k, "bytes")
    return host


def page_codecs(chunk, metas):
    """The leaf stream's codec byte of every nested page (behind its level header)."""
    out, pos = [], 0
    for m in metas:
        rep_len, def_len = np.frombuffer(chunk[pos + 4:pos + 12], np.uint32)
        out.append(chunk[pos + 12 + int(rep_len) + int(def_len)])
        pos += m.length
    return out


def options(codec=O.NONE, ratio=None, step=0, forced=-1):
    import pa_amd

    return pa_amd.WriteOptions(default_compression=codec, default_compress_ratio=ratio, max_page_size=step or None,
                               forced_codec=forced, seed=SEED)


# ---- the reference's integration shapes ---------------------------------------
def io_case(case):
    f, a = nestgen.io_rs_cases(np.random.default_rng(500 + IO_CASES.index(case)))[case]
    return f, a, 2048 if a.length > 2048 else 256


@pytest.mark.parametrize("codec", list(CODECS))
@pytest.mark.parametrize("case", IO_CASES)
def test_io_rs_shapes_equal_the_host_writer(ctx, case, codec):
    f, a, step = io_case(case)
    assert_same(f, a, options(CODECS[codec], 2.0, step), ctx, case)


@pytest.mark.parametrize("case", IO_CASES)
def test_io_rs_shapes_zstd_decode(ctx, case):
    import pa_amd

    f, a, step = io_case(case)
    host, dev = both(f, a, options(O.ZSTD, 2.0, step), ctx)
    for (hc, hm), (dc, dm) in zip(host, dev):
        assert [m.num_values for m in dm] == [m.num_values for m in hm]
        assert sum(m.length for m in dm) == len(dc)
        assert page_codecs(dc, dm) == page_codecs(hc, hm)
    pf = nestgen.pa_amd_field(f)
    dec = pa_amd.FieldDecoder(pf, dev, ctx)
    try:
        got = nestgen.device_to_host(f, dec.decode())
    finally:
        dec.close()
    NE.equal(f, got, NE.read_field(f, [(c, [(m.length, m.num_values) for m in pm]) for c, pm in host]),
             values_under_nulls=True)


# ---- every nest kind and level width ------------------------------------------
def deep_fields():
    i16 = nestgen.leaf("i16", True, "item")
    four = nestgen.lst(nestgen.lst(nestgen.lst(nestgen.lst(i16, True, "item"), True, "item"), True, "item"), True)
    mixed = nestgen.lst(nestgen.struct([
        nestgen.lst(nestgen.lst(nestgen.leaf("utf8", True, "item"), True, "item"), True, "l"),
        nestgen.leaf("bool", True, "b")], True, "item"), True)
    return {"four_lists_i16": four, "list_struct_list_list_utf8": mixed}


SHAPES = {**nestgen.shapes(), **deep_fields()}


@pytest.mark.parametrize("ratio", [None, 2.0], ids=["plain", "ratio2"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes_at_every_step(ctx, name, ratio):
    f = SHAPES[name]
    a = nestgen.gen(f, 600, np.random.default_rng(40 + list(SHAPES).index(name)))
    for step in STEPS:
        assert_same(f, a, options(O.NONE, ratio, step), ctx, (name, step))


def test_level_widths_of_the_deep_fields():
    """four nullable lists over a nullable leaf: rep width 3, def width 4."""
    import pa_amd

    path = nestgen.pa_amd_field(deep_fields()["four_lists_i16"]).leaf_paths()[0]
    nulls, mask, leaf_null, _ = pa_amd.nested.init_chain(path)
    max_rep = sum(1 for d in range(len(nulls)) if not (mask >> d) & 1)
    max_def = sum(nulls) + max_rep + leaf_null
    assert (max_rep.bit_length(), max_def.bit_length()) == (3, 4)


# ---- long and empty lists -----------------------------------------------------
def long_list_list(rng):
    n = 200
    outer = rng.integers(0, 40, n)
    ov = rng.random(n) > 0.1
    outer = np.where(ov, outer, 0)
    oo = np.zeros(n + 1, np.int64)
    oo[1:] = np.cumsum(outer)
    m = int(oo[-1])
    inner = rng.integers(0, 300, m)
    iv = rng.random(m) > 0.1
    inner = np.where(iv, inner, 0)
    io = np.zeros(m + 1, np.int64)
    io[1:] = np.cumsum(inner)
    k = int(io[-1])
    leaf = A("leaf", k, rng.random(k) > 0.2, values=rng.integers(0, 1000, k).astype(np.int32))
    f = nestgen.lst(nestgen.lst(nestgen.leaf("i32", True, "item"), True, "item"), True)
    return f, A("list", n, ov, offsets=oo, children=[A("list", m, iv, offsets=io, children=[leaf])])


@pytest.mark.parametrize("step", [1, 33, 0])
def test_long_lists(ctx, step):
    f, a = long_list_list(np.random.default_rng(3))
    host = assert_same(f, a, options(O.NONE, 2.0, step), ctx, step)
    if step == 0:
        assert host[0][1][0].num_values > 200_000  # far more levels in the page than rows


@pytest.mark.parametrize("ratio", [None, 2.0], ids=["plain", "ratio2"])
def test_empty_bool_lists(ctx, ratio):
    n = 3000
    f = nestgen.lst(nestgen.leaf("bool", True, "item"), True)
    a = A("list", n, np.random.default_rng(1).random(n) > 0.3, offsets=np.zeros(n + 1, np.int64),
          children=[A("leaf", 0, np.zeros(0, bool), values=np.zeros(0, bool))])
    host = assert_same(f, a, options(O.NONE, ratio, 700), ctx)
    assert [m.num_values for m in host[0][1]] == [700, 700, 700, 700, 200]


# ---- leaf families at ragged slices -------------------------------------------
@pytest.mark.parametrize("mode", ["lz4", "rle"])
@pytest.mark.parametrize("kind", ["bool", "utf8"])
def test_leaf_families_at_ragged_slices(ctx, kind, mode):
    f = nestgen.lst(nestgen.leaf(kind, True, "item"), True)
    a = nestgen.gen(f, 600, np.random.default_rng(8))
    starts = {int(a.offsets[r]) % 8 == 0 for r in range(0, 600, 33)}
    assert starts == {True, False}  # page slices start on a byte and inside one
    opts = options(O.LZ4, None, 33) if mode == "lz4" else options(O.NONE, None, 33, forced=RLE)
    assert_same(f, a, opts, ctx, (kind, mode))


def test_utf8_dict_and_freq_pages(ctx):
    f = nestgen.lst(nestgen.leaf("utf8", True, "item"), True)
    dict_a = nestgen.gen(f, 600, np.random.default_rng(9), uniq=50)
    freq_a = nestgen.gen(f, 600, np.random.default_rng(10), null_density=0.05, uniq=50)
    # most leaf slots null: the Freq rule's null share (compression/binary/mod.rs:312-320)
    freq_a.children[0].validity = np.random.default_rng(11).random(freq_a.children[0].length) > 0.95
    seen = set()
    for a in (dict_a, freq_a):
        for step in (0, 300):
            host = assert_same(f, a, options(O.LZ4, 2.0, step), ctx)
            seen |= set(page_codecs(*host[0]))
    assert {DICT, FREQ} <= seen


def test_largest_step(ctx):
    f = nestgen.lst(nestgen.leaf("i32", True, "item"), True)
    a = nestgen.gen(f, 40_000, np.random.default_rng(12))
    host = assert_same(f, a, options(O.LZ4, 2.0, 16384), ctx)
    assert len(host[0][1]) == 3


# ---- round trip in HBM --------------------------------------------------------
@pytest.mark.parametrize("case", ["test_struct_list", "test_list_map"])
def test_round_trip_in_hbm(ctx, case):
    import pa_amd

    f, a, step = io_case(case)
    pf = nestgen.pa_amd_field(f)
    opts = options(O.LZ4, 2.0, step)
    dec = pa_amd.FieldDecoder(pf, pa_amd.encode_field(pf, nestgen.host_array(a), opts), ctx)
    try:
        darr = dec.decode()
    finally:
        dec.close()
    dev = pa_amd.encode_field_device(pf, darr, opts, ctx)  # the decoded array as it is
    first = nestgen.device_to_host(f, darr)
    host = pa_amd.encode_field(pf, nestgen.host_array(first), opts)
    assert [(c.cpu().numpy().tobytes(), metas_of([(c, pm)])[0]) for c, pm in dev] == \
        [(c, metas_of([(c, pm)])[0]) for c, pm in host]
    dec = pa_amd.FieldDecoder(pf, dev, ctx)
    try:
        second = nestgen.device_to_host(f, dec.decode())
    finally:
        dec.close()
    NE.equal(f, second, first, values_under_nulls=True)


# ---- refusals -----------------------------------------------------------------
def small_list_list():
    f = nestgen.lst(nestgen.lst(nestgen.leaf("i32", False, "item"), False, "item"), False)
    n = 64
    oo = np.arange(0, 2 * n + 1, 2, dtype=np.int64)
    io = np.arange(0, 3 * 2 * n + 1, 3, dtype=np.int64)
    leaf = A("leaf", 6 * n, None, values=np.arange(6 * n, dtype=np.int32))
    return f, A("list", n, None, offsets=oo, children=[A("list", 2 * n, None, offsets=io, children=[leaf])])


@pytest.mark.parametrize("where", ["page_boundary", "inside_a_page"])
def test_decreasing_inner_offsets_are_refused(ctx, where):
    import pa_amd

    f, a = small_list_list()
    darr = pa_amd.device_array(nestgen.host_array(a), 0)
    row = 16 if where == "page_boundary" else 21  # pages of 16 rows
    b = int(a.offsets[row])
    io = darr.children[0].offsets
    io[b] = io[b - 1] - 1
    with pytest.raises(pa_amd.StrawboatError) as e:
        pa_amd.encode_field_device(nestgen.pa_amd_field(f), darr, options(step=16), ctx)
    assert e.value.status == 6


def test_nullable_nest_without_its_bitmap_is_refused(ctx):
    """The C entry point wants the bitmap of a nullable nest (the binding
    fills in an all-valid one for a validity of None, as encode_field reads
    it: io.rs's nullable structs carry none)."""
    import ctypes

    import pa_amd
    from pa_amd import _native as N
    from pa_amd import nested as NS

    n = 100
    offs = torch.arange(0, n + 1, dtype=torch.int64, device="cuda:0")
    vals = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    ones = torch.full((n,), 255, dtype=torch.uint8, device="cuda:0")
    out = torch.empty(1 << 16, dtype=torch.uint8, device="cuda:0")
    desc = NS.NestedDescC(N.INT32, 1, (ctypes.c_int32 * NS.MAX_NEST)(1, 0, 0, 0), 1, 4, 0)
    opts = options().c()
    metas = (N.PageMetaC * 4)()
    olen, npg = ctypes.c_uint64(), ctypes.c_uint64()

    def call(nest_bitmap, leaf_bitmap):
        nests = (NS.NestDevC * NS.MAX_NEST)()
        nests[0].d_offsets = offs.data_ptr()
        nests[0].d_validity = nest_bitmap
        return NS._encode_device_lib().sb_encode_nested_column_device(
            ctx._h, ctypes.byref(desc), nests, vals.data_ptr(), None, 0, leaf_bitmap, n, ctypes.byref(opts), 0,
            out.data_ptr(), out.numel(), ctypes.byref(olen), metas, 4, ctypes.byref(npg))

    assert call(None, ones.data_ptr()) == 6
    assert call(ones.data_ptr(), None) == 6
    assert call(ones.data_ptr(), ones.data_ptr()) == 0 and npg.value == 1 and metas[0].num_values == n


def test_depth_five_is_not_implemented(ctx):
    import pa_amd

    f = nestgen.leaf("i32", False, "item")
    for _ in range(5):
        f = nestgen.lst(f, False, "item")
    a = nestgen.gen(f, 20, np.random.default_rng(2))
    with pytest.raises(pa_amd.StrawboatError) as e:
        pa_amd.encode_field_device(nestgen.pa_amd_field(f), pa_amd.device_array(nestgen.host_array(a), 0), options(),
                                   ctx)
    assert e.value.status == 2


# ---- NativeWriter -------------------------------------------------------------
def test_native_writer_takes_a_device_array(ctx):
    import pa_amd

    f, a, step = io_case("test_struct")
    pf, ha = nestgen.pa_amd_field(f), nestgen.host_array(a)
    files = []
    for arr in (ha, pa_amd.device_array(ha, 0)):
        w = pa_amd.NativeWriter(options(O.LZ4, 2.0, step))
        w.start()
        w.write([(pf, arr)])
        files.append(w.finish())
    assert files[0] == files[1]
