"""GPU: the loop the two file readers share (egogaussian_amd/file_reader.py DeviceFileReader.decode), through each of them: a call of three
batches whose last holds a file the device refuses, then a call with a larger file on the same reader, so that its buffers grow."""
import numpy as np
import pytest

from tests import jpeg_cases as JC
from tests import png_decode_cases as DC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _png_case():
    from egogaussian_amd import png
    corpus = DC.corpus()
    fits = sorted((k for k, (_, img, _) in corpus.items() if img.shape[2] <= 130 and img.shape[1] <= 67), key=lambda k: (corpus[k][1].size, k))
    hwc = lambda k: np.ascontiguousarray(corpus[k][1].transpose(1, 2, 0))
    bad = next(iter(DC.malformed().values()))
    return png.PngReader, [(corpus[k][0], hwc(k)) for k in fits[:4]], (bad[0], bad[1]), (corpus[fits[-1]][0], hwc(fits[-1]))


def _jpeg_case():
    from egogaussian_amd import jpeg
    return (jpeg.JpegReader, [JC.golden()[n] for n in ("37x53-420-rb1", "31x15-L", "17x33-420", "37x53-L")], JC.malformed()["bytes left over"],
            JC.golden()["130x67-420"])


@pytest.mark.parametrize("case", [_png_case, _jpeg_case], ids=["PngReader", "JpegReader"])
def test_three_batches_with_a_refused_file_then_a_larger_file_on_the_same_reader(case):
    cls, good, (bad, status), (large, large_pixels) = case()
    rd = cls(DEV, batch=2, guard=256)
    with pytest.raises(ValueError, match=r"file 4: .*\(status %d\)" % status) as e:
        rd.read([g[0] for g in good] + [bad])
    assert str(e.value).startswith(cls.__name__ + ".read: file 4: ") and not any(f"file {k}" in str(e.value) for k in range(4))
    assert rd.last_status == [0, 0, 0, 0, status]
    for k, (_, pixels) in enumerate(good):
        assert np.array_equal(rd.last_results[k].cpu().numpy(), pixels), k
    assert len(rd.last_results) == 5 and bool((rd.last_results[4] == rd.GUARD_BYTE).all()), "a refused file receives no pixel"
    assert rd.host_reads == 3, "one read of the status words per batch"
    assert rd.check_guards()
    before = {k: rd._dev[k].numel() for k in ("out", "scratch")}
    # (the upload buffer is allocated in steps of 4096 bytes, and with these files the larger one does not cross a step: the first call's
    # largest batch uploads 7 152 bytes (JPEG) or 768 (PNG), the larger file alone 7 376 or 1 520.  So it is only held not to shrink.)
    blob_before = rd._dev["blob"].numel()
    out = rd.read([large])
    assert len(out) == 1 and np.array_equal(out[0].cpu().numpy(), large_pixels)
    assert rd.host_reads == 4
    assert rd.check_guards()
    assert rd.last_status == [0]
    assert all(rd._dev[k].numel() > before[k] for k in before), "the larger file did not make the buffers grow"
    assert rd._dev["blob"].numel() >= blob_before, "buffers only grow"
