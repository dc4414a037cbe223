"""Selective reads of List<primitive> columns on the GPU:
ListColumnDecoder.select against the oracle's full decode masked with numpy.

Every column lies on ragged pages (sellistgen), every selection of
selgen.selections is applied to it.  Per (column, selection): offsets, list
validity, leaf values and leaf validity equal the masked oracle result bit
for bit (bytes under null leaves included, bitmap bits past the last row /
leaf zero, offsets from 0 in the column's width), a 64-byte 0xA5 tail behind
every output (allocated at the plan's bound) is untouched, a second decode
of the same plan gives the same bytes, and the untouched pages' bytes are
never read."""
import ctypes

import numpy as np
import pytest

from tests import selgen as S
from tests import sellistgen as G

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TAIL = 64
NEST = [(True, True), (False, False), (True, False), (False, True)]
NEST_IDS = ["ln_in", "lr_ir", "ln_ir", "lr_in"]
_TDT = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _guarded(nbytes):
    """A device buffer of nbytes with a 0xA5 tail behind it -> (whole, view of the first nbytes)."""
    whole = torch.full((nbytes + TAIL,), 0xA5, dtype=torch.uint8, device="cuda")
    return whole, whole[:nbytes]


def _tail_ok(whole):
    return bool((whole[-TAIL:] == 0xA5).all())


def _selection(mask):
    import pa_amd

    return pa_amd.Selection(mask=torch.from_numpy(mask).cuda())


def _row_metas(col, rows=G.PAGE_ROWS):
    import pa_amd

    return [pa_amd.PageMeta(m.length, r) for m, r in zip(col["metas"], rows)]


def _decoder(col, sel, chunk, large=False, packed=False, dtype=None):
    import pa_amd

    return pa_amd.ListColumnDecoder.select(chunk, col["metas"], dtype if dtype is not None else col["dtype"],
                                           col["ln"], col["inn"], sel, large=large, packed=packed)


def _run(col, dec, exp, large=False):
    """One decode of `dec` into guarded buffers allocated at the plan's bound, compared with `exp`."""
    k, w, ow = exp["rows"], col["dtype"].itemsize, 8 if large else 4
    assert dec.num_rows == k
    assert dec.leaf_bound >= exp["leaves"]
    bound = dec.leaf_bound
    words = lambda n: 4 * max((n + 31) // 32, 1)  # noqa: E731
    ow_, o = _guarded((k + 1) * ow)
    vw, v = _guarded(max(bound, 1) * w)
    lw, lv = _guarded(words(k)) if col["ln"] else (None, None)
    fw, fv = _guarded(words(bound)) if col["inn"] else (None, None)
    go, gl, gv, gf = dec.decode(o.view(torch.int64 if large else torch.int32), lv, v.view(_TDT[w]), fv)
    torch.cuda.synchronize()
    assert dec.written_leaves() == exp["leaves"]
    assert go.cpu().numpy().tobytes() == exp["offsets"]
    assert gv.cpu().numpy().tobytes() == exp["values"]
    assert _tail_ok(ow_) and _tail_ok(vw)
    if col["ln"]:
        assert gl.cpu().numpy().tobytes()[:len(exp["list_validity"])] == exp["list_validity"]
        assert _tail_ok(lw)
    if col["inn"]:
        got = gf.cpu().numpy().tobytes()
        assert got[:len(exp["leaf_validity"])] == exp["leaf_validity"]
        # the words between the leaves written and the bound stay as the decode zeroed them
        assert not any(got[len(exp["leaf_validity"]):4 * ((bound + 31) // 32)])
        assert _tail_ok(fw)


def _untouched_ff(col, counts):
    """The device chunk with every untouched page's bytes overwritten by 0xFF."""
    raw = np.frombuffer(col["chunk"], np.uint8).copy()
    pos = 0
    for m, c in zip(col["metas"], counts):
        if not c:
            raw[pos:pos + m.length] = 0xFF
        pos += m.length
    return torch.from_numpy(raw).cuda()


def _packed(col, touched):
    import pa_amd

    raw = np.frombuffer(col["chunk"], np.uint8)
    parts = [raw[off:off + ln] for off, ln, _, _ in pa_amd.page_runs(col["metas"], touched)]
    return torch.from_numpy(np.concatenate(parts) if parts else np.zeros(1, np.uint8)).cuda()


def _check_column(col, large=False, names=None):
    chunk = torch.from_numpy(np.frombuffer(col["chunk"], np.uint8).copy()).cuda()
    for name, mask in S.selections(col["n"], col["bounds"]).items():
        if names is not None and name not in names:
            continue
        exp = G.expected(col, mask, large)
        touched = [i for i, c in enumerate(S.page_counts(mask, col["bounds"])) if c]
        dec = _decoder(col, _selection(mask), chunk, large)
        try:
            assert dec.num_pages == len(touched), name
            _run(col, dec, exp, large)
            _run(col, dec, exp, large)  # the plan's counters and the zeroed bitmaps are reset between decodes
            direct, compacted, scratch = dec.stats()
            assert (direct, compacted) == (0, len(touched)), name
            assert (scratch == 0) == (name == "none")
        finally:
            dec.close()


@pytest.mark.parametrize("large", [False, True], ids=["list", "large_list"])
@pytest.mark.parametrize("writer", S.WRITERS)
@pytest.mark.parametrize("nest", NEST, ids=NEST_IDS)
def test_select_list_int32_matches_masked_oracle(gpu, nest, writer, large):
    _check_column(G.column("int32", nest[0], nest[1], writer), large)


@pytest.mark.parametrize("dtype", ["int8", "int16", "int64", "float64"])
def test_select_list_widths_match_masked_oracle(gpu, dtype):
    _check_column(G.column(dtype, True, True, "adaptive"))


def test_select_list_page_rows_from_the_chunk(gpu):
    import pa_amd

    col = G.column()
    assert pa_amd.list_page_rows(col["chunk"], col["metas"]) == list(G.PAGE_ROWS)
    short = [pa_amd.PageMeta(m.length, m.num_values) for m in col["metas"][:2]] + [pa_amd.PageMeta(11, 1)]
    with pytest.raises(pa_amd.StrawboatError) as e:
        pa_amd.list_page_rows(col["chunk"], short)
    assert (e.value.status, e.value.page) == (pa_amd._native.E_IO, 2)


def test_select_list_all_equals_the_full_decode(gpu):
    import pa_amd

    col = G.column()
    full = pa_amd.ListColumnDecoder(col["chunk"], col["metas"], col["dtype"], True, True)
    fo, fl, fv, ff = full.decode()
    rows, leaves = full.num_rows, full.num_leaves
    got = pa_amd.read_selected_list(col["chunk"], col["metas"], col["dtype"], True, True,
                                    _selection(np.ones(col["n"], bool)))
    torch.cuda.synchronize()
    # (the full decode leaves the bits past the last row / leaf of its bitmaps undefined: whole bytes, then the bits)
    bits = lambda t, n: (t.cpu().numpy()[:n // 8].tobytes(),  # noqa: E731
                         np.unpackbits(t.cpu().numpy()[n // 8:n // 8 + 1], bitorder="little")[:n % 8].tolist())
    assert got[0].cpu().numpy().tobytes() == fo.cpu().numpy().tobytes() and got[0].numel() == rows + 1
    assert got[2].cpu().numpy().tobytes() == fv[:leaves].cpu().numpy().tobytes() and got[2].numel() == leaves
    assert bits(got[1], rows) == bits(fl, rows)
    assert bits(got[3], leaves) == bits(ff, leaves)
    full.close()


def test_select_list_untouched_pages_are_never_read(gpu):
    import pa_amd

    col = G.column()
    mask = S.selections(col["n"], col["bounds"])["holes"]
    exp = G.expected(col, mask)
    counts = S.page_counts(mask, col["bounds"])
    touched = [i for i, c in enumerate(counts) if c]
    assert len(touched) < len(counts)
    # resolved against the page rows beforehand: the plan itself reads no byte
    # of an untouched page, its row count included
    res = _selection(mask).resolve(_row_metas(col))
    try:
        assert res.pages == touched
        dec = _decoder(col, res, _untouched_ff(col, counts))
        try:
            _run(col, dec, exp)
            assert dec.num_pages == len(touched)
        finally:
            dec.close()
        packed = _packed(col, touched)
        assert packed.numel() == sum(r[1] for r in pa_amd.page_runs(col["metas"], res.pages)) < len(col["chunk"])
        dec = _decoder(col, res, packed, packed=True)
        try:
            _run(col, dec, exp)
        finally:
            dec.close()
    finally:
        res.close()


def _corrupt_codec(col, page):
    """The chunk with the codec byte of `page`'s values stream (behind the level streams) set to 99."""
    raw = np.frombuffer(col["chunk"], np.uint8).copy()
    pos, _, rep_len, def_len = G.page_header(col["chunk"], col["metas"])[page]
    raw[pos + 12 + rep_len + def_len] = 99
    return torch.from_numpy(raw).cuda()


def test_select_list_errors_name_the_columns_page(gpu):
    import pa_amd

    col = G.column()
    sels = S.selections(col["n"], col["bounds"])
    for name, page in (("holes", 7), ("holes", 9), ("bernoulli_0.5", 8)):
        counts = S.page_counts(sels[name], col["bounds"])
        assert counts[page] and any(counts[:page])  # touched, and not the first touched page
        with pytest.raises(pa_amd.StrawboatError) as e:
            dec = _decoder(col, _selection(sels[name]), _corrupt_codec(col, page))
            try:
                dec.decode()
            finally:
                dec.close()
        assert e.value.page == page, (name, str(e.value))
        assert e.value.status in (pa_amd._native.E_OUT_OF_SPEC, pa_amd._native.E_NYI, pa_amd._native.E_CODEC)
    for page in (0, 5, len(col["metas"]) - 1):  # the same corruption on an untouched page: never seen
        dec = _decoder(col, _selection(sels["holes"]), _corrupt_codec(col, page))
        try:
            _run(col, dec, G.expected(col, sels["holes"]))
        finally:
            dec.close()


def test_select_list_wrong_page_rows_fail_the_plan(gpu):
    import pa_amd

    col = G.column()
    rows = list(G.PAGE_ROWS)
    rows[3] -= 1  # one row moved from page 3 to page 4: the sum stays
    rows[4] += 1
    res = _selection(np.ones(col["n"], bool)).resolve(_row_metas(col, rows))
    try:
        with pytest.raises(pa_amd.StrawboatError) as e:
            _decoder(col, res, col["chunk"])
        assert (e.value.status, e.value.page) == (pa_amd._native.E_ARG, 3), str(e.value)
    finally:
        res.close()


def test_select_list_general_walk_fallback(gpu):
    """Level streams of far more than 64 hybrid runs (what k_list's run table
    holds) send the inner list plan to the general level walk; the take
    works on its scratch unchanged."""
    import pa_amd
    from pa_amd.nested import _nested_lib

    col = G.walk_column()
    assert col["max_runs"] > 64
    # a list plan of these pages is a plan of the general walk (only such a one counts nested levels)
    for c, walk in ((col, True), (G.column(), False)):
        full = pa_amd.ListColumnDecoder(c["chunk"], c["metas"], c["dtype"], True, True)
        assert _nested_lib().sb_plan_nested_count(full._h, 0) == (G.N_ROWS if walk else 0)
        full.close()
    _check_column(col, names=("range", "bernoulli_0.5"))


def test_select_list_argument_checks(gpu):
    import pa_amd
    from pa_amd.nested import ListOutC

    E = pa_amd._native
    col = G.column()
    ones = np.ones(col["n"], bool)
    with pytest.raises(pa_amd.StrawboatError) as e:  # an unresolved Selection cannot know a packed chunk's pages
        _decoder(col, _selection(ones), col["chunk"], packed=True)
    assert e.value.status == E.E_ARG
    with pytest.raises(pa_amd.StrawboatError) as e:
        _decoder(col, _selection(ones[:-1]), col["chunk"])
    assert e.value.status == E.E_ARG
    for leaf in (pa_amd.UTF8, np.bool_):
        with pytest.raises(pa_amd.StrawboatError) as e:
            _decoder(col, _selection(ones), col["chunk"], dtype=leaf)
        assert e.value.status == E.E_NYI
    dec = _decoder(col, _selection(ones), col["chunk"])
    full = pa_amd.ListColumnDecoder(col["chunk"], col["metas"], col["dtype"], True, True)
    try:
        o, lv, v, fv = dec.alloc_outputs()
        for outs in ((o, None, v, fv), (o, lv, None, fv), (o, lv, v, None)):
            with pytest.raises(pa_amd.StrawboatError) as e:
                dec.decode_async(*outs)
            assert e.value.status == E.E_ARG
        out = ListOutC(o.data_ptr(), lv.data_ptr(), v.data_ptr(), fv.data_ptr())
        L = pa_amd.lib()
        assert L.sb_decode_list_planned(dec.ctx._h, dec._h, ctypes.byref(out)) == E.E_ARG
        assert L.sb_decode_list_selected(full.ctx._h, full._h, ctypes.byref(out)) == E.E_ARG
        n = ctypes.c_uint64()
        assert L.sb_plan_selected_leaves(full.ctx._h, full._h, ctypes.byref(n)) == E.E_ARG
    finally:
        dec.close()
        full.close()


def test_select_list_empty_selection(gpu):
    import pa_amd

    col = G.column()
    for large in (False, True):
        o, lv, v, fv = pa_amd.read_selected_list(col["chunk"], col["metas"], col["dtype"], True, True,
                                                 pa_amd.Selection(ranges=[], n_rows=col["n"]), large=large)
        assert o.cpu().numpy().tolist() == [0] and v.numel() == 0
        assert o.dtype == (torch.int64 if large else torch.int32)
        assert not lv.cpu().numpy().any() and not fv.cpu().numpy().any()


def test_select_list_from_a_file(gpu, tmp_path):
    import pa_amd

    pa = pytest.importorskip("pyarrow")
    col = G.column()
    item = pa.field("item", pa.int32(), True)
    schema = pa.schema([pa.field("l", pa.list_(item), True),
                        pa.field("ll", pa.list_(pa.field("item", pa.list_(item), True)), True)])
    p = tmp_path / "lists.sb"
    # (the depth-2 column is refused by its schema before a byte of it is read)
    p.write_bytes(pa_amd.assemble_file([(col["chunk"], col["metas"])] * 2, schema.serialize().to_pybytes()[8:]))
    sels = S.selections(col["n"], col["bounds"])
    with pa_amd.StrawboatFile(p) as f:
        assert [l.depth for l in f.leaves] == [1, 2]
        assert f.page_rows(0) == list(G.PAGE_ROWS)
        for name in ("range", "holes", "none", "all"):
            mask = sels[name]
            exp = G.expected(col, mask)
            touched = [i for i, c in enumerate(S.page_counts(mask, col["bounds"])) if c]
            o, lv, v, fv = f.read_selected_list(0, _selection(mask))
            torch.cuda.synchronize()
            assert f.last_uploaded_bytes == sum(r[1] for r in pa_amd.page_runs(col["metas"], touched)), name
            assert o.cpu().numpy().tobytes() == exp["offsets"], name
            assert v.cpu().numpy().tobytes() == exp["values"], name
            assert lv.cpu().numpy().tobytes()[:len(exp["list_validity"])] == exp["list_validity"], name
            assert fv.cpu().numpy().tobytes()[:len(exp["leaf_validity"])] == exp["leaf_validity"], name
        with pytest.raises(pa_amd.StrawboatError) as e:
            f.read_selected_list(1, _selection(sels["range"]))
        assert e.value.status == pa_amd._native.E_NYI
