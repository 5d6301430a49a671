"""GPU: batched device JPEG decode (rtdm.jpeg.BatchDecoder / decode_batch: one plan, threaded
Huffman stage, one copy, rtdm_jpeg_reconstruct_batch's two launches) bit-exact against
Pillow's libjpeg-turbo decode and against the single-image rtdm.jpeg.decode: every fixture
and variant (4:4:4 / 4:2:2 / 4:2:0 / gray, restart markers, 1x1 .. 33x31, sizes that are no
MCU multiple) in ONE call, BGR, n = 1, same-size batches as one [N, H, W, 3] tensor,
caller-provided pitched output, buffer reuse and regrowth without a host synchronise,
strict / non-strict refusal, and cli.load_images."""
import io

import numpy as np
import pytest
import torch

from jpeg_cases import FIXTURES, pillow_rgb, progressive, variants

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def cases():
    """(name, bytes, Pillow's RGB decode): the reference, computed once and left unchanged"""
    out = [(f.rsplit("/", 1)[1], open(f, "rb").read()) for f in FIXTURES] + variants()
    out = [(name, d, pillow_rgb(d)) for name, d in out]
    for _, _, want in out:
        want.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def pair240(cases):
    """the 240 x 240 fixture and a different-quality re-encode of it: (bytes, Pillow's decode) x 2"""
    from PIL import Image
    _, d, want = next(c for c in cases if c[2].shape == (240, 240, 3))
    b = io.BytesIO()
    Image.fromarray(want).save(b, "JPEG", quality=60)
    return (d, want), (b.getvalue(), pillow_rgb(b.getvalue()))


def _tiny(cases):
    return [c for c in cases if "x" in c[0] and not c[0].endswith(".jpg")]


def _same(got, want, name=""):
    got = got.cpu().numpy()
    assert got.shape == want.shape, (name, got.shape, want.shape)
    assert np.array_equal(got, want), (name, int((got != want).sum()))


def test_all_cases_in_one_call(dev, cases):
    from rtdm import jpeg as J
    assert len(cases) > 25
    datas = [d for _, d, _ in cases]
    rgb = J.decode_batch(datas, dev)
    bgr = J.decode_batch(datas, dev, bgr=True)
    torch.cuda.synchronize()
    assert len(rgb) == len(bgr) == len(cases) and rgb.stacked is None
    for (name, _, want), a, b in zip(cases, rgb, bgr):
        _same(a, want, name)
        _same(b, want[..., ::-1], name + " bgr")


def test_small_batches_equal_single_decode(dev, cases):
    """n = 1, and batches of the tiny variants (1 to 40 blocks per image: no multiple of the
    256-block IDCT workgroup, so every image ends inside a partly used workgroup)"""
    from rtdm import jpeg as J
    tiny = [(name, d) for name, d, _ in _tiny(cases)]
    assert len(tiny) == 12
    dec = J.BatchDecoder(dev, threads=2)
    one = dec.decode([tiny[3][1]])
    few = dec.decode([d for _, d in tiny])
    big = dec.decode([cases[0][1]])
    single = [J.decode(d, dev) for _, d in tiny]
    torch.cuda.synchronize()
    assert len(one) == 1 and torch.equal(one[0], single[3])
    for (name, _), a, b in zip(tiny, few, single):
        assert a.shape == b.shape and torch.equal(a, b), name
    _same(big[0], cases[0][2])
    assert big.stacked.shape == (1,) + cases[0][2].shape  # one image is a batch of one size


def test_same_size_batch_is_one_tensor(dev, pair240):
    from rtdm import jpeg as J
    (d, _), (d2, want2) = pair240
    datas = [d, d2, d]
    out = J.decode_batch(datas, dev)
    singles = torch.stack([J.decode(x, dev) for x in datas])
    torch.cuda.synchronize()
    assert out.stacked is not None and out.stacked.shape == (3, 240, 240, 3) and out.stacked.is_contiguous()
    assert torch.equal(out.stacked, singles)
    assert all(out[i].data_ptr() == out.stacked[i].data_ptr() for i in range(3))
    _same(out.stacked[1], want2)
    assert not torch.equal(out.stacked[0], out.stacked[1])


def test_caller_provided_pitched_out(dev, cases, pair240):
    from rtdm import jpeg as J
    (d0, w0), (d1, w1) = pair240
    h, w = w0.shape[:2]
    # rows of a wider canvas: 5 sentinel pixels right of every image row, 2 sentinel rows below
    canvas = torch.full((2, h + 2, w + 5, 3), 0xA5, dtype=torch.uint8, device=dev)
    out = canvas[:, :h, :w]
    res = J.decode_batch([d0, d1], dev, out=out)
    torch.cuda.synchronize()
    assert res.stacked is out and res[1].data_ptr() == out[1].data_ptr()
    got = canvas.cpu().numpy()
    assert np.array_equal(got[0, :h, :w], w0) and np.array_equal(got[1, :h, :w], w1)
    assert (got[:, h:] == 0xA5).all() and (got[:, :, w:] == 0xA5).all()
    # a list of per-image tensors of different sizes, one of them with pitched rows (an odd
    # pitch: its rows start at every byte alignment)
    name, dv, wv = next(c for c in cases if c[0] == "422_17x9")
    wide = torch.full((9, 23, 3), 0x5A, dtype=torch.uint8, device=dev)
    plain = torch.full((h, w, 3), 0x5A, dtype=torch.uint8, device=dev)
    res = J.decode_batch([dv, d0], dev, out=[wide[:, :17], plain])
    torch.cuda.synchronize()
    got = wide.cpu().numpy()
    assert np.array_equal(got[:, :17], wv) and (got[:, 17:] == 0x5A).all()
    _same(plain, w0)
    assert res.stacked is None
    with pytest.raises(ValueError):
        J.decode_batch([dv, d0], dev, out=[plain, plain])  # shapes do not match the images
    with pytest.raises(ValueError):
        J.decode_batch([d0], "cpu")


def test_reuse_and_regrowth_without_sync(dev, cases):
    from rtdm import jpeg as J
    dec = J.BatchDecoder(dev, threads=3)
    tiny = _tiny(cases)
    first = dec.decode([d for _, d, _ in tiny[:4]])
    second = dec.decode([d for _, d, _ in tiny[4:9]])
    small_bytes = dec._stage.numel(), dec._ws.numel()
    # large enough to regrow every buffer: all fixtures, three times over, with no sync between
    tiny_names = {c[0] for c in tiny}
    large_cases = [c for c in cases if c[0] not in tiny_names] * 3
    third = dec.decode([d for _, d, _ in large_cases])
    fourth = dec.decode([d for _, d, _ in tiny[9:]])
    assert dec._stage.numel() > small_bytes[0] and dec._ws.numel() > small_bytes[1]
    torch.cuda.synchronize()
    for res, ref in ((first, tiny[:4]), (second, tiny[4:9]), (third, large_cases), (fourth, tiny[9:])):
        assert len(res) == len(ref)
        for got, (name, _, want) in zip(res, ref):
            _same(got, want, name)


def test_strict_and_non_strict_refusal(dev, cases):
    from rtdm import _lib as L
    from rtdm import jpeg as J
    (_, d0, w0), (_, d1, w1) = cases[0], cases[20]
    res = J.decode_batch([d0, progressive(), d1, b"\x00junk"], dev, strict=False)
    torch.cuda.synchronize()
    assert res[1] is None and res[3] is None and res.stacked is None
    _same(res[0], w0)
    _same(res[2], w1)
    # refused by the Huffman stage, after the plan gave it blocks and workgroups (a scan that
    # names Huffman table 4): the kernels skip it, its neighbours are untouched
    pos = 2
    while d0[pos + 1] != 0xDA:
        pos += 2 + ((d0[pos + 2] << 8) | d0[pos + 3])
    bad = d0[:pos + 6] + b"\x40" + d0[pos + 7:]
    res = J.decode_batch([d1, bad, d0], dev, strict=False)
    torch.cuda.synchronize()
    assert res[1] is None
    _same(res[0], w1)
    _same(res[2], w0)
    with pytest.raises(L.RtdmError, match="image 1: jpeg: scan names"):
        J.decode_batch([d1, bad, d0], dev)
    with pytest.raises(NotImplementedError, match="image 1"):
        J.decode_batch([d0, progressive(), d1], dev)
    with pytest.raises(L.RtdmError, match="image 2"):
        J.decode_batch([d0, d1, b"\xff\xd8\xff\xd9"], dev)
    assert J.decode_batch([], dev) == []


def test_cli_load_images(dev, cases, tmp_path):
    from PIL import Image
    from rtdm import cli
    paths = []
    for i, data in enumerate((cases[0][1], None, progressive(), cases[2][1])):
        p = tmp_path / (f"img{i}.png" if data is None else f"img{i}.jpg")
        if data is None:
            Image.fromarray(np.ascontiguousarray(cases[1][2][:50, :70])).save(p)
        else:
            p.write_bytes(data)
        paths.append(str(p))
    frames = cli.load_images(paths, dev)
    singles = [cli.load_image(p, dev) for p in paths]
    torch.cuda.synchronize()
    assert len(frames) == 4
    for a, b in zip(frames, singles):
        assert a.dtype == torch.uint8 and a.shape == b.shape and torch.equal(a, b)
    _same(frames[0], cases[0][2])
    _same(frames[3], cases[2][2])
