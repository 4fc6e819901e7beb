"""GPU: bfhip_jpeg_decode (csrc/jpeg.hip) against its restatement jpeg.torch_jpeg_decode and against the recorded Pillow pixels,
bit for bit.  No PIL needed: the streams and pixels come from tests/golden/jpeg_cases.npz."""
import hashlib

import numpy as np
import pytest
import torch

import jpeg_cases as jc

pytestmark = pytest.mark.gpu

STREAMS = jc.streams()


@pytest.fixture(scope="module")
def jpeg():
    from bevfusion_amd import jpeg
    return jpeg


@pytest.fixture(scope="module")
def mixed(jpeg, dev):
    """Every recorded stream entropy-decoded, and ONE device call over all of them: frames of different sizes, sampling and
    tables.  (frames, device views, the flat buffer with a guard band)."""
    frames = [jpeg.entropy_decode(data) for _, data, _ in STREAMS]
    views, flat = jpeg.fused_decode_batch(frames, dev, guard=256)
    torch.cuda.synchronize()
    return frames, views, flat


def test_mixed_batch_equals_restatement(jpeg, mixed):
    frames, views, _ = mixed
    assert len({(h.hs[0], h.vs[0]) for h, _ in frames}) == 3 and len({(h.width, h.height) for h, _ in frames}) == 6
    for (name, _, _), (h, coef), got in zip(STREAMS, frames, views):
        assert got.dtype == torch.uint8 and tuple(got.shape) == (h.height, h.width, 3)
        assert torch.equal(got.cpu(), jpeg.torch_jpeg_decode(h, coef)), name


def test_mixed_batch_equals_recorded_pillow_pixels(mixed):
    _, views, _ = mixed
    for (name, _, pixels), got in zip(STREAMS, views):
        assert np.array_equal(got.cpu().numpy(), pixels), name


def test_partial_mcus_write_exactly_h_by_w_pixels(mixed):
    frames, views, flat = mixed
    total = sum(h.height * h.width * 3 for h, _ in frames)
    assert flat.numel() == total + 256
    assert bool((flat[total:] == 0xA5).all())  # nothing behind the last frame (1x1, 9x7, 17x23: partial MCUs on both edges)
    at = 0
    for (h, _), v in zip(frames, views):  # the frames follow one another densely: a frame that overran would show in the next
        assert v.data_ptr() == flat.data_ptr() + at
        at += h.height * h.width * 3


@pytest.mark.parametrize("w,h,hs,vs", [(17, 23, 2, 2), (9, 7, 1, 1), (19, 10, 2, 1), (10, 19, 1, 2), (3, 5, 2, 2)],
                         ids=["420_17x23", "444_9x7", "422_19x10", "440_10x19", "420_3x5_replicated"])
def test_full_range_coefficients_pin_the_wraparound(jpeg, dev, w, h, hs, vs):
    """Random int16 blocks over the whole range with random 8-bit tables: where no encoder goes, the kernel and the
    restatement still agree, because both are 32-bit wrap-around."""
    rs = np.random.RandomState(w * 100 + h)
    frames = []
    for k in range(4):
        header = jpeg.make_header(w, h, hs, vs, rs.randint(1, 256, (3, 64)))
        coef = rs.randint(-32768, 32768, header.coef_bytes // 2).astype(np.int16)
        if k == 3:
            coef[::2] = rs.choice([-32768, 32767], coef[::2].size).astype(np.int16)
        frames.append((header, coef))
    views, _ = jpeg.fused_decode_batch(frames, dev)
    for (header, coef), got in zip(frames, views):
        want = jpeg.torch_jpeg_decode(header, coef)
        assert torch.equal(got.cpu(), want)
    assert len({bytes(v.cpu().numpy().tobytes()) for v in views}) == 4


def test_fixture_frame_full_size(jpeg, dev):
    z = jc.load()
    header, coef = jpeg.entropy_decode(open(jc.FIXTURE, "rb").read())
    H, W = header.height, header.width
    assert (H, W) == (900, 1600) and header.block_rows[0] * 8 == 912
    (got,), flat = jpeg.fused_decode_batch([(header, coef)], dev, guard=4096)
    (again,), _ = jpeg.fused_decode_batch([(header, coef)], dev)
    assert bool((flat[H * W * 3:] == 0xA5).all())
    assert tuple(got.shape) == (H, W, 3)
    assert torch.equal(got, again)  # two runs, identical bytes
    host = got.cpu()
    assert torch.equal(host, jpeg.torch_jpeg_decode(header, coef))
    px = host.numpy()
    assert np.array_equal(px[:32, :32], z["fixture_window_top_left"])
    assert np.array_equal(px[H - 32:, W - 32:], z["fixture_window_bottom_right"])
    assert np.array_equal(px[H // 2 - 16:H // 2 + 16, W // 2 - 16:W // 2 + 16], z["fixture_window_centre"])
    assert hashlib.sha256(np.ascontiguousarray(px).tobytes()).hexdigest() == str(z["fixture_sha256"])


def test_bad_descriptors_are_refused_before_any_launch(jpeg, dev):
    """A plane buffer smaller than the frame's planes: BFHIP_E_INVALID from the host-side validation, nothing launched."""
    header, coef = jpeg.entropy_decode(STREAMS[0][1])
    need = sum(header.block_cols[c] * header.block_rows[c] * 64 for c in range(3))
    with pytest.raises(ValueError):
        jpeg.fused_decode_batch([(header, coef)], dev, planes=torch.empty(need - 64, dtype=torch.uint8, device=dev))
    from bevfusion_amd import _lib
    import ctypes
    d = jpeg._Frame()
    d.width, d.height, d.hs, d.vs = header.width, header.height, header.hs[0], header.vs[0]
    at = 0
    for c in range(3):
        d.coef_off[c], d.plane_off[c] = header.coef_offset[c], at
        d.block_cols[c], d.block_rows[c] = header.block_cols[c], header.block_rows[c]
        at += header.block_cols[c] * header.block_rows[c] * 64
    buf = torch.empty(1 << 16, dtype=torch.uint8, device=dev)
    args = lambda planes_bytes, rgb_bytes, coef_elems: (ctypes.addressof(d), buf.data_ptr(), 1, buf.data_ptr(), coef_elems,  # noqa: E731
                                                        buf.data_ptr(), planes_bytes, buf.data_ptr(), rgb_bytes, None)
    lib = _lib.load()
    ok_rgb = header.width * header.height * 3
    assert lib.bfhip_jpeg_decode(*args(need - 1, ok_rgb, header.coef_bytes // 2)) == -1
    assert lib.bfhip_jpeg_decode(*args(need, ok_rgb - 1, header.coef_bytes // 2)) == -1
    assert lib.bfhip_jpeg_decode(*args(need, ok_rgb, header.coef_bytes // 2 - 1)) == -1
    d.hs = 3
    assert lib.bfhip_jpeg_decode(*args(need, ok_rgb, header.coef_bytes // 2)) == -1


def synthetic_frames(jpeg, seed, n, w, h):
    """JpegFrames made without a file: smooth random blocks of modest size at 4:2:0."""
    rs = np.random.RandomState(seed)
    headers, coefs = [], []
    for _ in range(n):
        header = jpeg.make_header(w, h, 2, 2, rs.randint(1, 20, (3, 64)))
        coef = np.zeros(header.coef_bytes // 2, np.int16).reshape(-1, 64)
        coef[:, 0] = rs.randint(-60, 60, coef.shape[0])
        coef[:, 1:10] = rs.randint(-8, 9, (coef.shape[0], 9))
        headers.append(header)
        coefs.append(coef.reshape(-1))
    offsets = np.concatenate([[0], np.cumsum([c.size for c in coefs])])
    return jpeg.JpegFrames(headers, np.concatenate(coefs), offsets)


@pytest.mark.parametrize("with_plan", [True, False], ids=["img_aug_plan", "no_plan"])
def test_preprocessor_with_jpeg_frames_equals_the_eager_path(jpeg, dev, monkeypatch, with_plan):
    """2 samples x 2 views of a 40 x 56 frame: JpegFrames through Det3DDataPreprocessor against the decoded blocks through the
    same module, on the fused decoder and with BFHIP_JPEG_DECODE=0."""
    from bevfusion_amd import data_preprocessor as dp
    from bevfusion_amd import image_aug as ia
    H, W, N = 40, 56, 2
    samples = [synthetic_frames(jpeg, 10 + b, N, W, H) for b in range(2)]
    blocks = [s.decode_host() for s in samples]
    assert blocks[0].shape == (N, H, W, 3) and not torch.equal(blocks[0], blocks[1]) and blocks[0].float().std() > 5
    mod = dp.Det3DDataPreprocessor(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], pad_size_divisor=32).to(dev)
    inputs = {}
    if with_plan:
        aug = ia.ImageAug3D(final_dim=[24, 32], resize_lim=[0.7, 0.9], bot_pct_lim=[0.0, 0.0], rot_lim=[-5.4, 5.4], rand_flip=True,
                            is_train=True, defer=True)
        cam2img = np.tile(np.array([[30.0, 0, 28, 0], [0, 30, 20, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float32), (N, 1, 1))
        cam2lidar = np.tile(np.eye(4), (N, 1, 1))
        cam2lidar[:, 2, :3] = (0.0, -1.0, 0.0)
        np.random.seed(7)
        inputs["img_aug_plan"] = [aug.transform(dict(img=s, ori_shape=(H, W), cam2img=cam2img, cam2lidar=cam2lidar))["img_aug_plan"]
                                  for s in samples]
        eager = blocks
    else:
        eager = [b.permute(0, 3, 1, 2) for b in blocks]
    want = mod(dict(inputs=dict(inputs, img=eager)))["inputs"]["imgs"]
    before = dict(jpeg.PATHS)
    got = mod(dict(inputs=dict(inputs, img=samples)))["inputs"]["imgs"]
    assert jpeg.PATHS["kernel"] == before["kernel"] + 1 and jpeg.PATHS["torch"] == before["torch"]
    assert got.shape == want.shape == ((2, N, 3, 32, 32) if with_plan else (2, N, 3, 64, 64))
    assert torch.equal(got, want)
    monkeypatch.setattr(jpeg, "ENABLED", False)  # BFHIP_JPEG_DECODE=0
    off = mod(dict(inputs=dict(inputs, img=samples)))["inputs"]["imgs"]
    assert jpeg.PATHS["torch"] == before["torch"] + 1
    assert torch.equal(off, want)
