"""Selective reads on the GPU: ColumnDecoder.select / BinaryColumnDecoder.select
against the oracle's full-column decode masked with numpy.

Every column has ragged pages (selgen.PAGE_ROWS), every selection of
selgen.selections is applied to it.  Per (column, selection): the buffers
equal the masked oracle result bit for bit (values under nulls included,
bitmap bits past the last row zero, offsets from 0 in the column's width),
a 64-byte 0xA5 tail behind every output is untouched, a second decode of the
same plan gives the same bytes, the untouched pages' bytes are never read
(they are overwritten with 0xFF; a packed buffer of the touched runs gives
the same result), and fixed-width / Boolean plans compact exactly the
partially selected pages."""
import numpy as np
import pytest

from tests import selgen as S

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TAIL = 64


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


def _selection(name, mask):
    """The mask as a pa_amd.Selection, through each of its three constructors."""
    import pa_amd

    n = len(mask)
    if name in ("range", "first", "last", "none"):  # as ranges
        d = np.diff(np.concatenate([[0], mask.astype(np.int8), [0]]))
        rs = list(zip(np.flatnonzero(d == 1).tolist(), np.flatnonzero(d == -1).tolist()))
        return pa_amd.Selection(ranges=rs[::-1] + [(3, 3)], n_rows=n, device="cuda")
    if name == "alternate":  # as a packed device bitmap
        bits = torch.from_numpy(np.packbits(mask, bitorder="little")).cuda()
        return pa_amd.Selection(mask=bits, n_rows=n)
    return pa_amd.Selection(mask=torch.from_numpy(mask).cuda())


def _decoder(col, sel, chunk, packed=False):
    import pa_amd

    if "eo" in col:
        return pa_amd.BinaryColumnDecoder.select(chunk, col["metas"], col["phys"], col["nullable"], sel, packed=packed)
    dt = np.bool_ if col["kind"] == "bool" else np.dtype(col["kind"])
    return pa_amd.ColumnDecoder.select(chunk, col["metas"], dt, col["nullable"], sel, packed=packed)


def _run(col, dec, exp):
    """One decode of `dec` into guarded buffers, compared with `exp`."""
    k = exp["rows"]
    assert dec.num_rows == k
    words = 4 * max((k + 31) // 32, 1)
    mw, m = _guarded(words) if col["nullable"] else (None, None)
    if "eo" in col:
        ow = col["ow"]
        cap = max(dec.values_bytes, 16)
        ow_, o = _guarded((k + 1) * ow)
        vw, v = _guarded(cap)
        o = o.view(torch.int32 if ow == 4 else torch.int64)
        go, gv, gm = dec.decode(o, v, m)
        torch.cuda.synchronize()
        assert dec.written_bytes() == len(exp["values"])
        assert go.cpu().numpy().tobytes() == exp["offsets"]
        assert gv.cpu().numpy().tobytes() == exp["values"]
        assert _tail_ok(ow_) and _tail_ok(vw)
    else:
        if col["kind"] == "bool":
            vw, v = _guarded(words)
            nbytes = 4 * ((k + 31) // 32)
        else:
            w = np.dtype(col["kind"]).itemsize
            vw, v = _guarded(max(k, 1) * w)
            v = v.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[w])
            nbytes = k * w
        gv, gm = dec.decode(v, m)
        torch.cuda.synchronize()
        assert gv.cpu().numpy().tobytes()[:nbytes] == exp["values"]
        assert _tail_ok(vw)
    if col["nullable"]:
        assert gm.cpu().numpy().tobytes()[:len(exp["validity"])] == exp["validity"]
        assert _tail_ok(mw)


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


@pytest.mark.parametrize("writer", S.WRITERS)
@pytest.mark.parametrize("nullable", [False, True])
@pytest.mark.parametrize("kind", S.KINDS)
def test_select_matches_masked_oracle(gpu, kind, nullable, writer):
    col = S.column(kind, nullable, writer)
    for name, mask in S.selections(col["n"], col["bounds"]).items():
        exp = S.expected(col, mask)
        counts = S.page_counts(mask, col["bounds"])
        touched = [i for i, c in enumerate(counts) if c]
        sel = _selection(name, mask)
        res = sel.resolve(col["metas"])
        assert (res.num_rows, res.pages, res.counts) == (exp["rows"], touched, [c for c in counts if c]), name
        res.close()
        dec = _decoder(col, sel, _untouched_ff(col, counts))
        try:
            assert dec.num_pages == len(touched)
            _run(col, dec, exp)
            _run(col, dec, exp)  # the plan's counters and zeroed bitmaps are reset between decodes
            direct, compacted, scratch = dec.stats()
            if "eo" not in col:
                partial = sum(1 for c, nv in zip(counts, S.PAGE_ROWS) if 0 < c < nv)
                assert (direct, compacted) == (len(touched) - partial, partial), name
                if name == "all":
                    assert (compacted, scratch) == (0, 0)
            if name == "none":
                assert (direct, compacted, scratch) == (0, 0, 0)
        finally:
            dec.close()
        dec = _decoder(col, sel, _packed(col, touched), packed=True)
        try:
            _run(col, dec, exp)
        finally:
            dec.close()


def test_select_page_above_65536_rows(gpu):
    col = S.column("int32", True, "adaptive", page_rows=(70000,))
    rng = np.random.default_rng(9)
    half = rng.random(70000) < 0.5
    tail = np.zeros(70000, bool)
    tail[65000:69999] = True
    for mask in (half, tail):
        import pa_amd

        dec = _decoder(col, pa_amd.Selection(mask=torch.from_numpy(mask).cuda()), col["chunk"])
        try:
            _run(col, dec, S.expected(col, mask))
            assert dec.stats()[:2] == (0, 1)
        finally:
            dec.close()


def test_select_empty_returns_empty_arrays(gpu):
    import pa_amd

    sel_mask = np.zeros(S.N_ROWS, bool)
    col = S.column("int64", True, "adaptive")
    v, m = pa_amd.read_selected(col["chunk"], col["metas"], np.int64, True, pa_amd.Selection(ranges=[], n_rows=S.N_ROWS))
    assert v.numel() == 0 and not m.cpu().numpy().any()
    col = S.column("utf8", True, "adaptive")
    o, v, m = pa_amd.read_selected(col["chunk"], col["metas"], pa_amd.UTF8, True,
                                   pa_amd.Selection(mask=torch.from_numpy(sel_mask)))
    assert o.cpu().numpy().tolist() == [0] and v.numel() == 0 and o.dtype == torch.int32
    col = S.column("large_binary", False, "lz4")
    o, v, m = pa_amd.read_selected(col["chunk"], col["metas"], pa_amd.LARGE_BINARY, False,
                                   pa_amd.Selection(mask=torch.from_numpy(sel_mask)))
    assert o.cpu().numpy().tolist() == [0] and v.numel() == 0 and o.dtype == torch.int64 and m is None


def _corrupt_codec(col, page):
    """The chunk with the codec byte of `page`'s value stream set to 99."""
    raw = np.frombuffer(col["chunk"], np.uint8).copy()
    pos = sum(m.length for m in col["metas"][:page])
    if col["nullable"]:
        pos += 4 + int.from_bytes(raw[pos:pos + 4].tobytes(), "little")
    raw[pos] = 99
    return torch.from_numpy(raw).cuda()


@pytest.mark.parametrize("kind,nullable", [("int32", False), ("int64", True), ("bool", True), ("utf8", True)])
def test_select_errors_name_the_columns_page(gpu, kind, nullable):
    import pa_amd

    col = S.column(kind, nullable, "adaptive")
    sels = S.selections(col["n"], col["bounds"])
    # pages 0, 5 and the last are untouched by "holes": page 7 is compacted, page 9 decoded in place
    for name, page in (("holes", 7), ("holes", 9), ("bernoulli_0.5", 8)):
        counts = S.page_counts(sels[name], col["bounds"])
        assert counts[page] and any(counts[:page])  # touched, and not the first touched page
        with pytest.raises(pa_amd.StrawboatError) as e:
            dec = _decoder(col, pa_amd.Selection(mask=torch.from_numpy(sels[name]).cuda()), _corrupt_codec(col, page))
            try:
                dec.decode()
            finally:
                dec.close()
        assert e.value.page == page, (name, str(e.value))
        assert e.value.status in (pa_amd._native.E_OUT_OF_SPEC, pa_amd._native.E_NYI, pa_amd._native.E_CODEC)
    for page in (0, 5, len(col["metas"]) - 1):  # the same corruption on an untouched page: never read
        dec = _decoder(col, pa_amd.Selection(mask=torch.from_numpy(sels["holes"]).cuda()), _corrupt_codec(col, page))
        try:
            _run(col, dec, S.expected(col, sels["holes"]))
        finally:
            dec.close()


def test_select_rejects_a_selection_of_another_length(gpu):
    import pa_amd

    col = S.column("int32", False, "adaptive")
    with pytest.raises(pa_amd.StrawboatError) as e:
        pa_amd.Selection(mask=torch.ones(S.N_ROWS - 1, dtype=torch.bool)).resolve(col["metas"])
    assert e.value.status == pa_amd._native.E_ARG


def test_select_nested_leaf_is_not_implemented(gpu, tmp_path):
    import pa_amd

    pa = pytest.importorskip("pyarrow")
    offs = np.arange(0, 33, 2).astype(np.int64)
    cols = [pa_amd.encode_list_column(offs, np.arange(32, dtype=np.int64), None, None, False, False)]
    schema = pa.schema([pa.field("l", pa.list_(pa.field("item", pa.int64(), False)), False)])
    p = tmp_path / "nested.sb"
    p.write_bytes(pa_amd.assemble_file(cols, schema.serialize().to_pybytes()[8:]))
    with pa_amd.StrawboatFile(p) as f:
        with pytest.raises(pa_amd.StrawboatError) as e:
            f.read_selected(0, pa_amd.Selection(ranges=[(0, 4)], n_rows=16))
        assert e.value.status == pa_amd._native.E_NYI
