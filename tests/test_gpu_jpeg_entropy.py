"""JPEG entropy decoding on the GPU (rt_set_jpeg_entropy mode 1, retto_amd/csrc/jpeg_huff.hip) against the host decoder, whose
coefficients, pixels and error texts are the reference: exact, no tolerance."""
import numpy as np
import pytest

import retto_amd
from retto_amd import workload
from test_jpeg_entropy_cpu import CASES, assert_same_planes, case_file, jpeg

pytestmark = pytest.mark.gpu


@pytest.fixture
def entropy_session(hip_session):
    hip_session.set_jpeg_entropy(1)
    yield hip_session
    hip_session.set_jpeg_entropy(0)


@pytest.mark.parametrize("name", sorted(CASES))
def test_kernel_coefficients_equal_host_decoder(hip_session, name):
    data = case_file(name)
    ref, _ = retto_amd.debug_jpeg_entropy(data, 0)
    got, info = hip_session.debug_jpeg_entropy(data, 1)
    print(name, info)
    assert info["taken"] == 1 and info["flag"] == 0
    assert_same_planes(got, ref)
    if name == "1x1":
        assert info["subsequences"] == 1
    if name == "several_workgroups":   # the link pass and the scan across workgroups ran
        assert info["workgroups"] > 1 and info["link_rounds"] >= 1


def test_public_path_with_device_entropy(entropy_session):
    s = entropy_session
    assert s.jpeg_entropy == 1
    files = [case_file(n) for n in sorted(CASES)]
    import io
    from PIL import Image
    png = io.BytesIO()
    Image.fromarray(np.random.default_rng(5).integers(0, 256, (33, 47, 3), dtype=np.uint8)).save(png, "PNG")
    mixed = files + [jpeg(67, 93, quality=90, progressive=True), png.getvalue()]
    pages, dev, ent = s.decode_batch(mixed, with_entropy=True)
    for f, p in zip(mixed, pages):
        assert np.array_equal(p, retto_amd.decode_image(f))
    assert ent == [2] * len(files) + [1, 0]
    # text pages through the pipeline: mode 1 reads what mode 0 reads
    enc = []
    for i in range(5):
        b = io.BytesIO()
        Image.fromarray(workload.planted_page(224, 320, 4, seed=40 + i)[0]).save(b, "JPEG", quality=90, subsampling=2)
        enc.append(b.getvalue())
    got = s.wait_batch(s.submit_encoded_batch(enc))
    s.set_jpeg_entropy(0)
    ref = s.wait_batch(s.submit_encoded_batch(enc))
    assert len(got) == len(ref) == 5
    for g, r in zip(got, ref):
        assert [x.text for x in g.rec_result] == [x.text for x in r.rec_result]
        assert [x.score for x in g.rec_result] == [x.score for x in r.rec_result]
        assert len(g.det_result) == len(r.det_result)
        for d, e in zip(g.det_result, r.det_result):
            assert np.array_equal(d.boxes.as_array(), e.boxes.as_array()) and d.score == e.score


@pytest.mark.parametrize("damage", ["byte", "cut"])
def test_damaged_streams_go_the_hosts_way(entropy_session, damage):
    good = case_file("one_workgroup")
    sos = good.index(b"\xff\xda")
    mid = (sos + len(good)) // 2
    bad = good[:mid] + bytes([good[mid] ^ 0x5A]) + good[mid + 1:] if damage == "byte" else good[:len(good) // 3]

    _, info = entropy_session.debug_jpeg_entropy(bad, 1)
    print(damage, info)
    # the changed byte reaches the kernels and comes back flagged (the host-fallback branch); the cut file has no marker behind
    # its entropy data, so the preparation refuses it
    assert (info["taken"], info["flag"]) == ((1, 1) if damage == "byte" else (0, 0))

    def outcome(fn):
        try:
            return "pixels", fn()
        except retto_amd.RettoError as e:
            return "error", str(e)

    ref = outcome(lambda: retto_amd.decode_image(bad))
    got = outcome(lambda: entropy_session.decode_batch([bad])[0][0])
    assert got[0] == ref[0]
    assert np.array_equal(got[1], ref[1]) if ref[0] == "pixels" else got[1] == ref[1]
    pages, _, ent = entropy_session.decode_batch([good], with_entropy=True)   # the session's next call succeeds
    assert ent == [2] and np.array_equal(pages[0], retto_amd.decode_image(good))
