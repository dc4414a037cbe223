"""The device nested writers (pa_amd.encode_field_device,
encode_list_column_device) and the nested decoder on legal Arrow arrays
outside the normal form of nestgen.gen -- tests/test_nested_loose_cpu.py on
the GPU: a dead list / map slot that is not empty is refused by the check
kernel (k_nest_check / k_enc_list_levels) with SB_E_ARG, the accepted loose
arrays give the host writer's bytes and decode to their logical value
(nestgen.logical, pinned against pyarrow on the CPU), and a nested page whose
leaf stream holds more values than its levels give leaf slots is refused by
the decoder."""
import numpy as np
import pytest

from oracle import nest as NE
from oracle import oracle as O
from tests import nestgen

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SEED = 13
E_OUT_OF_SPEC, E_ARG = 1, 6


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pa_amd

    return pa_amd.default_context(0)


def options(codec=O.NONE, ratio=None, step=0):
    import pa_amd

    return pa_amd.WriteOptions(default_compression=codec, default_compress_ratio=ratio, max_page_size=step or None,
                               seed=SEED)


def flat(cols):
    """[(chunk, metas)] -> [(bytes, [(length, num_values)])]."""
    return [(c if isinstance(c, bytes) else c.cpu().numpy().tobytes(), [(m.length, m.num_values) for m in pm])
            for c, pm in cols]


def both(f, a, opts, ctx):
    import pa_amd

    pf, ha = nestgen.pa_amd_field(f), nestgen.host_array(a)
    return pa_amd.encode_field(pf, ha, opts), pa_amd.encode_field_device(pf, pa_amd.device_array(ha, 0), opts, ctx)


def decoded(f, cols, ctx):
    import pa_amd

    dec = pa_amd.FieldDecoder(nestgen.pa_amd_field(f), cols, ctx)
    try:
        return nestgen.device_to_host(f, dec.decode())
    finally:
        dec.close()


# ---- 5. refusals --------------------------------------------------------------------
@pytest.mark.parametrize("row", nestgen.DEAD_ROWS)
@pytest.mark.parametrize("case", list(nestgen.dead_fields()))
def test_dead_slot_with_children_is_refused(ctx, case, row):
    import pa_amd

    f, bad, twin = nestgen.dead_case(case, row)
    pf, opts = nestgen.pa_amd_field(f), options(step=16)
    with pytest.raises(pa_amd.StrawboatError) as e:
        pa_amd.encode_field_device(pf, pa_amd.device_array(nestgen.host_array(bad), 0), opts, ctx)
    assert e.value.status == E_ARG and "not empty" in str(e.value)
    host, dev = both(f, twin, opts, ctx)  # the twin: the same array with that one range empty
    assert flat(dev) == flat(host)
    if case == "top_list":
        up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")  # noqa: E731
        ch = bad.children[0]
        with pytest.raises(pa_amd.StrawboatError) as e:
            pa_amd.encode_list_column_device(up(bad.offsets), up(ch.values), up(bad.validity), up(ch.validity), True, True,
                                             opts, ctx)
        assert e.value.status == E_ARG and "not empty" in str(e.value)
        ch = twin.children[0]
        got = pa_amd.encode_list_column_device(up(twin.offsets), up(ch.values), up(twin.validity), up(ch.validity), True,
                                               True, opts, ctx)
        assert flat([got]) == flat(host)


# ---- 6. the device writer equals the host writer on loose arrays ---------------------
@pytest.mark.parametrize("codec", ["none", "lz4"])
@pytest.mark.parametrize("shape", list(nestgen.loose_shapes()))
def test_loose_arrays_equal_the_host_writer_and_decode(ctx, shape, codec):
    f, a = nestgen.loose_array(shape)
    lg = nestgen.logical(f, a)
    if shape == "list_bool":  # page 0's Boolean leaf slice starts inside a byte
        assert a.offsets[0] % 8 != 0
    for step in (7, 33, 0):
        host, dev = both(f, a, options(O.LZ4 if codec == "lz4" else O.NONE, None, step), ctx)
        assert flat(dev) == flat(host), (shape, step)
        NE.equal(f, decoded(f, dev, ctx), lg, values_under_nulls=False, path=f"{shape}/{step}")


def test_loose_list_under_a_ratio(ctx):
    f, a = nestgen.loose_array("list_utf8")
    for step in (33, 0):
        host, dev = both(f, a, options(O.NONE, 2.0, step), ctx)
        assert flat(dev) == flat(host), step
        NE.equal(f, decoded(f, dev, ctx), nestgen.logical(f, a), values_under_nulls=False)


# ---- 7. no rows, one row ---------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1])
def test_empty_and_one_row(ctx, n):
    f = nestgen.shapes()["list_null_struct_list"]
    a = nestgen.gen(f, n, np.random.default_rng(5))
    host, dev = both(f, a, options(O.LZ4, None, 16), ctx)
    assert flat(dev) == flat(host)
    assert [len(pm) for _, pm in host] == [n] * len(host)


# ---- 8. the decoder: more leaf values than leaf slots ---------------------------------
def test_page_with_surplus_leaf_values_is_refused(ctx):
    """Page 1 of 4 of a List<Int32> column rebuilt from its own level header
    and a values stream two values longer than its levels give leaf slots
    (what a writer emits that keeps the children of a null slot).  The
    fixed-width None stream's byte count is compared with the slot count
    before any value is read (run_leaf), so only an under-read is at stake."""
    import pa_amd

    f = nestgen.lst(nestgen.leaf("i32", True, "item"), True)
    a = nestgen.gen(f, 64, np.random.default_rng(21))
    (path,) = NE.leaf_paths(f)
    (chunk, metas), = NE.write_field(f, a, 16)
    assert len(metas) == 4
    off = metas[0][0]
    rep, dfl, j0, j1 = NE.levels(a, path, 16, 32)
    leaf = a.children[0]
    assert j1 + 2 <= leaf.length
    max_rep, max_def = NE._max_levels(path)
    head = NE._levels_page(rep, dfl, max_rep, max_def, 16)

    def page(extra):
        e = j1 + extra
        return head + O.compress(np.ascontiguousarray(leaf.values[j0:e]), np.asarray(leaf.validity[j0:e], bool),
                                 O.WriteOptions.make())

    assert page(0) == chunk[off:off + metas[1][0]]  # the rebuilt page is the writer's
    bad = page(2)
    chunk2 = chunk[:off] + bad + chunk[off + metas[1][0]:]
    metas2 = [metas[0], (len(bad), metas[1][1])] + metas[2:]
    with pytest.raises(O.OracleError) as oe:
        NE.read_field(f, [(chunk2, metas2)])
    assert oe.value.code == E_OUT_OF_SPEC
    pm = lambda ms: [pa_amd.PageMeta(*m) for m in ms]  # noqa: E731
    NE.equal(f, decoded(f, [(chunk, pm(metas))], ctx), a, values_under_nulls=False)
    with pytest.raises(pa_amd.StrawboatError) as e:
        decoded(f, [(chunk2, pm(metas2))], ctx)
    assert e.value.status == E_OUT_OF_SPEC
    with pytest.raises(pa_amd.StrawboatError) as e:
        dec = pa_amd.NestedColumnDecoder(chunk2, pm(metas2), np.int32, (True,), True, ctx)
        try:
            dec.decode()
        finally:
            dec.close()
    assert e.value.status == E_OUT_OF_SPEC and "page 1" in str(e.value)
