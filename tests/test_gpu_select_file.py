"""StrawboatFile.read_selected: only the runs of touched pages leave the disk.
A three-column file (Int32, nullable Utf8, Boolean) whose untouched pages
are overwritten with 0xFF on disk still reads back the masked oracle result,
and last_uploaded_bytes is the sum of the touched pages' lengths."""
import numpy as np
import pytest

from tests import selgen as S

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
pa = pytest.importorskip("pyarrow")


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.mark.parametrize("name", ["range", "bernoulli_0.02"])
def test_file_read_selected(gpu, tmp_path, name):
    import pa_amd

    cols = [S.column("int32", False, "adaptive"), S.column("utf8", True, "adaptive"), S.column("bool", False, "lz4")]
    mask = S.selections(S.N_ROWS, S.BOUNDS)[name]
    counts = S.page_counts(mask, S.BOUNDS)
    assert 0 in counts and any(counts)
    schema = pa.schema([pa.field("a", pa.int32(), False), pa.field("s", pa.utf8(), True),
                        pa.field("b", pa.bool_(), False)])
    data = bytearray(pa_amd.assemble_file([(c["chunk"], c["metas"]) for c in cols],
                                          schema.serialize().to_pybytes()[8:]))
    p = tmp_path / "sel.sb"
    p.write_bytes(bytes(data))
    with pa_amd.StrawboatFile(p) as f:  # the untouched pages of every column: 0xFF on disk
        for c, cm in enumerate(f.columns):
            assert [(m.length, m.num_values) for m in cm.pages] == [(m.length, m.num_values) for m in cols[c]["metas"]]
            pos = cm.offset
            for m, k in zip(cm.pages, counts):
                if not k:
                    data[pos:pos + m.length] = b"\xff" * m.length
                pos += m.length
    p.write_bytes(bytes(data))
    sel = pa_amd.Selection(mask=torch.from_numpy(mask).cuda())
    with pa_amd.StrawboatFile(p) as f:
        for c, col in enumerate(cols):
            exp = S.expected(col, mask)
            out = f.read_selected(c, sel)
            torch.cuda.synchronize()
            assert f.last_uploaded_bytes == sum(m.length for m, k in zip(col["metas"], counts) if k)
            if "eo" in col:
                o, v, m = out
                assert o.cpu().numpy().tobytes() == exp["offsets"] and v.cpu().numpy().tobytes() == exp["values"]
            else:
                v, m = out
                assert v.cpu().numpy().tobytes()[:len(exp["values"])] == exp["values"]
            if col["nullable"]:
                assert m.cpu().numpy().tobytes()[:len(exp["validity"])] == exp["validity"]
