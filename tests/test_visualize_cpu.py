"""CPU: the specification of bevfusion_amd.visualize -- geometry against the reference's recorded projection, coverage against
hand-written canvases, the overflow trap, the mosaic and BEV cases, the tracker's recorded sequence, the registry and the tool."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import visualize_cases as cases
from bevfusion_amd import visualize as vz
from bevfusion_amd.registry import VISUALIZERS

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
U = 2.0 ** -24  # unit roundoff of float32


def gamma(k):
    return k * U / (1 - k * U)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "visualize_ref.npz"))


def tiled(frames, cam_order=None, scale=1):
    """The mosaic of the untouched frames, written independently of the module: cells, black remainder, block means."""
    N, H, W, _ = frames.shape
    order = list(range(N)) if cam_order is None else cam_order
    cols = 3 if len(order) > 2 else len(order)
    rows = -(-len(order) // cols)
    h, w = H // scale, W // scale
    out = np.zeros((rows * h, cols * w, 3), np.uint8)
    for i, v in enumerate(order):
        blk = frames[v][:h * scale, :w * scale].astype(np.int64).reshape(h, scale, w, scale, 3).sum((1, 3))
        out[(i // cols) * h:(i // cols + 1) * h, (i % cols) * w:(i % cols + 1) * w] = (blk + scale * scale // 2) // (scale * scale)
    return out


def affine_bound(M, p, e_p):
    """|fl(((M0 p0 + M1 p1) + M2 p2) + M3) - exact| for inputs p known to e_p: the inputs' errors through |M|, plus at most four
    roundings (one product, three sums) on every term's way to the result."""
    M, p = np.abs(M.astype(np.float64)), np.abs(p.astype(np.float64))
    return (M[..., :3] * e_p[..., None, :]).sum(-1) + gamma(4) * ((M[..., :3] * p[..., None, :]).sum(-1) + M[..., 3])


def test_corners_and_projection_against_the_reference(golden):
    """The float32 specification against the reference's float64 corners and project_to_image, within a running rounding-error
    bound computed from the inputs: cos and sin are rounded once and then pass one product and two sums (gamma_4 on |lx c| +
    |ly s| + |x|), each affine map adds the inputs' errors through |M| and gamma_4 of its terms, the quotient (e_0 + |u| e_2) /
    |h_2| plus its own rounding, plus the reference's 1e-8 in the divisor."""
    boxes, L, K = golden["boxes"], golden["lidar2cam"], golden["cam2img"]
    got = vz.box_corners(boxes)
    assert got.dtype == np.float32 and got.shape == (len(boxes), 8, 3)
    b = np.abs(boxes.astype(np.float64))
    lx, ly = b[:, 3] / 2, b[:, 4] / 2
    c, s = np.abs(np.cos(boxes[:, 6].astype(np.float64))), np.abs(np.sin(boxes[:, 6].astype(np.float64)))
    e_c = np.stack([gamma(4) * (lx * c + ly * s + b[:, 0]), gamma(4) * (lx * s + ly * c + b[:, 1]), gamma(1) * (b[:, 5] + b[:, 2])], -1)
    err = np.abs(got.astype(np.float64) - golden["corners"])
    assert (err <= e_c[:, None, :]).all(), (err / e_c[:, None, :]).max()
    assert err.max() > 0  # float32 really is in play

    uv, z = vz.project_corners(got, L, K)
    K34 = vz.as_cam2img(K)
    p = got.astype(np.float64)[None]                                     # [1, n, 8, 3]
    e_p = np.broadcast_to(e_c[None, :, None, :], p.shape)
    Lm = L[:, None, None, :3, :]                                         # [N, 1, 1, 3, 4]
    e_q = affine_bound(Lm, p, e_p)                                       # [N, n, 8, 3]
    q = (Lm[..., :3].astype(np.float64) * p[..., None, :]).sum(-1) + Lm[..., 3]
    assert (np.abs(z - golden["z_cam"]) <= e_q[..., 2]).all()
    near_zero = np.abs(golden["z_cam"]) <= e_q[..., 2]
    assert not near_zero.any()                                           # the generator's condition: no flag may differ
    assert np.array_equal(z > 0, golden["valid"])
    Km = K34[:, None, None]
    e_h = affine_bound(Km, q, e_q)
    h = (Km[..., :3].astype(np.float64) * q[..., None, :]).sum(-1) + Km[..., 3]
    ref = golden["uv"]
    h2 = np.abs(h[..., 2:3]) - e_h[..., 2:3]
    assert (h2 > 0).all()
    bound = (e_h[..., :2] + np.abs(ref) * e_h[..., 2:3]) / h2
    bound = bound + U * (np.abs(ref) + bound) + np.abs(ref) * 1e-8 / h2
    err = np.abs(uv.astype(np.float64) - ref)
    assert (err <= bound).all(), (err / bound).max()
    seen = golden["valid"] & (ref[..., 0] >= 0) & (ref[..., 0] < 1600) & (ref[..., 1] >= 0) & (ref[..., 1] < 900)
    assert seen.sum() >= 40 and (bound[seen] < 0.01).all()  # inside the frames the bound itself is far below a pixel


def test_cam2img_shapes_agree():
    kw = cases.camera_case("front")
    K = kw["cam2img"]
    k34 = np.concatenate([K, np.zeros((1, 3, 1), np.float32)], 2)
    k44 = np.concatenate([k34, np.array([[[0, 0, 0, 1]]], np.float32)], 1)
    want = vz.render_cameras(**kw)
    assert (want.numpy() != kw["frames"][0]).any()
    for k in (k34, k44):
        assert torch.equal(vz.render_cameras(**dict(kw, cam2img=k)), want)


@pytest.mark.parametrize("name", sorted(cases.COVERAGE))
def test_coverage_against_hand_written_canvas(name):
    img = vz.render_bev(**cases.coverage_case(name)).numpy()
    want = cases.canvas(cases.COVERAGE[name][2])
    red = (img == np.array([255, 0, 0], np.uint8)).all(-1)
    assert np.array_equal(red, want), "\n" + "\n".join("".join(".#"[int(v)] for v in row) for row in red)
    assert (img[~want] == 0).all()


def clipped_line64(kw):
    """The trap's segment in float64 from the specification's float32 corners: near clip, projection, pixel ends."""
    p = vz.box_corners(kw["boxes"]).astype(np.float64)[0]
    a, b = p[0], p[4]  # dy = dz = 0: corners 0..3 coincide, 4..7 coincide
    L, K = kw["lidar2cam"][0].astype(np.float64), kw["cam2img"][0].astype(np.float64)
    qa, qb = L[:3, :3] @ a + L[:3, 3], L[:3, :3] @ b + L[:3, 3]
    assert 0 < qa[2] - kw["near"] < 2e-3 and qb[2] > 1  # one end about 1 mm in front of the near plane
    ha, hb = K @ qa, K @ qb
    return ha[:2] / ha[2], hb[:2] / hb[2]


def test_overflow_trap_crosses_the_frame_where_the_float64_line_does():
    """An end about 750 000 pixels left of a 12 x 16 frame: squared cross products of such coordinates overflow 64 bits.  The
    drawn pixels are those within thickness / 2 of the float64 line.  Slack 0.1 pixel: the ends are rounded to 1/16 pixel (1/32),
    the guard clip rounds once more (1/32), and the float32 error of the far end (a few pixels at 750 000) reaches the frame
    scaled by frame width / segment length, below 1e-3."""
    kw = cases.trap_case()
    A, B = clipped_line64(kw)
    assert A[0] < -500000 and 0 < B[0] < 16 and 0 < B[1] < 12
    img = vz.render_cameras(**kw).numpy()
    ys, xs = np.mgrid[0:12, 0:16]
    P = np.stack([xs + 0.5, ys + 0.5], -1)
    d = B - A
    tt = np.clip(((P - A) @ d) / (d @ d), 0, 1)
    dist = np.linalg.norm(P - (A + tt[..., None] * d), axis=-1)
    red = (img == np.array([255, 0, 0], np.uint8)).all(-1)
    r = kw["thickness"] / 2
    assert red[dist < r - 0.1].all() and not red[dist > r + 0.1].any()
    assert red.sum() >= 12 and red[:, 0].any()  # it really crosses, from the left border on
    assert np.array_equal(img[~red], kw["frames"][0][~red])


@pytest.mark.parametrize("name", ["behind", "n0", "nan"])
def test_nothing_to_draw_returns_the_tiled_input(name):
    kw = cases.camera_case(name)
    assert np.array_equal(vz.render_cameras(**kw).numpy(), tiled(kw["frames"]))


def test_across_the_near_plane_is_clipped_not_dropped():
    kw = cases.camera_case("across")
    img = vz.render_cameras(**kw).numpy()
    red = (img == 255 * np.array([1, 0, 0], np.uint8)).all(-1) & (kw["frames"][0] != img).any(-1)
    assert red.sum() > 20
    far = vz.render_cameras(**dict(kw, near=7.0)).numpy()  # the whole box lies below this plane
    assert np.array_equal(far, kw["frames"][0])


def test_later_box_wins_and_swapping_flips():
    a, b = cases.camera_case("overlap"), cases.camera_case("overlap_swapped")
    ia, ib = vz.render_cameras(**a).numpy(), vz.render_cameras(**b).numpy()
    only_red = vz.render_cameras(**dict(a, boxes=a["boxes"][:1], colors=a["colors"][:1])).numpy()
    only_green = vz.render_cameras(**dict(a, boxes=a["boxes"][1:], colors=a["colors"][1:])).numpy()
    src = a["frames"][0]
    red, green = (only_red != src).any(-1), (only_green != src).any(-1)
    both = red & green
    assert both.sum() >= 4
    assert (ia[both] == [0, 255, 0]).all() and (ib[both] == [255, 0, 0]).all()
    assert np.array_equal(ia[~both], ib[~both])


def test_grid_and_cam_order():
    kw = cases.camera_case("five_views")
    img = vz.render_cameras(**kw).numpy()
    assert img.shape == (50, 111, 3) and (img[25:, 74:] == 0).all()
    empty = vz.render_cameras(**dict(kw, boxes=kw["boxes"][:0], colors=kw["colors"][:0])).numpy()
    assert np.array_equal(empty, tiled(kw["frames"])) and (img != empty).any()
    kw = cases.camera_case("three_views_order")
    plain = vz.render_cameras(**dict(kw, cam_order=None)).numpy()
    got = vz.render_cameras(**kw).numpy()
    for cell, view in enumerate(kw["cam_order"]):
        assert np.array_equal(got[:, cell * 37:(cell + 1) * 37], plain[:, view * 37:(view + 1) * 37])
    two = vz.render_cameras(**cases.camera_case("two_views"))
    assert tuple(two.shape) == (25, 74, 3)
    assert vz.infer_grid(1) == (1, 1) and vz.infer_grid(6) == (2, 3) and vz.infer_grid(7) == (3, 3)


@pytest.mark.parametrize("scale", [1, 2, 3])
def test_scale_is_the_rounded_block_mean_of_the_full_composite(scale):
    kw = cases.camera_case("scale%d" % scale)
    full = vz.render_cameras(**dict(kw, scale=1)).numpy()
    assert (full != tiled(kw["frames"])).any()
    got = vz.render_cameras(**kw).numpy()
    assert got.shape == (25 // scale, 2 * (37 // scale), 3)
    views = np.stack([full[:, :37], full[:, 37:]], 0)
    assert np.array_equal(got, tiled(views, scale=scale))


def test_bev_points_limits_duplicates_nan_and_row_flip():
    img = vz.render_bev(**cases.bev_case("limits")).numpy()
    want = np.zeros((12, 16), bool)
    for col, row in ((0, 11), (15, 0), (7, 0), (3, 7), (3, 7), (9, 10)):  # (x, y) -> (floor x, 11 - floor y); the others are outside
        # or have a non-finite x or y; the last has a NaN z, which a plot of x and y (the reference's scatter) never reads
        want[row, col] = True
    assert np.array_equal((img == 255).all(-1), want) and (img[~want] == 0).all()
    img = vz.render_bev(**cases.bev_case("point_size")).numpy()
    want = np.zeros((12, 16), bool)
    want[11, 0:2] = want[0:2, 15] = True   # squares of 2 span [c, c + 1] x [r, r + 1], cut at the canvas
    want[5:7, 8:10] = True
    assert np.array_equal((img == 255).all(-1), want)


def test_bev_footprint_is_drawn_over_the_points():
    kw = cases.bev_case("footprint_over_point")
    img = vz.render_bev(**kw).numpy()
    assert (img[5, 4] == [0, 255, 0]).all() and (img[9, 12] == 255).all()
    green = (img == np.array([0, 255, 0], np.uint8)).all(-1)
    want = np.zeros((12, 16), bool)
    # vertical edges at u = 4.5 and 9.5 (centres of columns 4 and 9), v from 4 to 7: rows 4 .. 6 beside them, and the caps reach
    # the centres of rows 3 and 7 (0.5 away, inclusive); horizontal edges at v = 4 and v = 7 (row borders): the rows on both sides
    want[3:8, 4] = want[3:8, 9] = True
    want[3:5, 4:10] = want[6:8, 4:10] = True
    assert np.array_equal(green, want), "\n" + "\n".join("".join(".#"[int(v)] for v in row) for row in green)


def test_bev_cloud_shape_and_default_thickness():
    kw = cases.bev_case("cloud")
    img = vz.render_bev(**kw)
    assert tuple(img.shape) == (120, 150, 3) and vz.bev_shape((-50, 50), (-50, 50), 10) == (1000, 1000)
    assert vz.DEFAULT_BEV_THICKNESS == 3.5 and vz.default_camera_thickness(1600) == 142 / 16


def test_palette():
    got = vz.palette_colors(np.array([0, 2, 1, 7]), ["car", "wheelbarrow", "pedestrian"])
    assert got.tolist() == [[255, 158, 0], [0, 0, 230], [255, 255, 255], [255, 255, 255]]


def test_tracker_follows_the_recorded_sequence(golden):
    tr = vz.Tracker3D(max_missed=3, max_dist=4.0)
    doff, off = golden["trk_det_off"], golden["trk_off"]
    assert len(doff) == 9 and doff[3] == doff[4]  # eight frames, the fourth empty
    for f in range(8):
        res = tr.update(golden["trk_dets"][doff[f]:doff[f + 1]])
        assert [r["id"] for r in res] == golden["trk_ids"][off[f]:off[f + 1]].tolist(), f
        assert np.array_equal(np.array([r["box"] for r in res], np.float32).reshape(-1, 9), golden["trk_boxes"][off[f]:off[f + 1]]), f


def test_select_and_visualize_sample():
    kw = cases.camera_case("overlap")
    pred = dict(bboxes_3d=torch.from_numpy(np.concatenate([kw["boxes"], np.zeros((2, 2), np.float32)], 1)),
                scores_3d=torch.tensor([0.9, 0.005]), labels_3d=torch.tensor([0, 8]))
    meta = dict(ori_cam2img=kw["cam2img"], lidar2cam=kw["lidar2cam"])
    classes = ["car"] + ["x%d" % i for i in range(7)] + ["pedestrian"]
    vis = VISUALIZERS.build(dict(type="PredictionVisualizer", classes=classes, thickness=1.5, xlim=(0, 16), ylim=(-6, 6), px_per_m=1))
    mosaic, bev = vis(meta, kw["frames"], np.zeros((0, 3), np.float32), dict(pred_instances_3d=pred))
    want = vz.render_cameras(**dict(kw, boxes=kw["boxes"][:1], colors=np.array([[255, 158, 0]], np.uint8)))
    assert torch.equal(mosaic, want) and tuple(bev.shape) == (12, 16, 3)
    assert [t["id"] for t in vis.tracker.get_results()] == [1]
    boxes, labels = vz.select_boxes(dict(gt_bboxes_3d=kw["boxes"], gt_labels_3d=np.array([0, 8])), only=[8])
    assert np.array_equal(boxes, kw["boxes"][1:]) and labels.tolist() == [8]


def test_paths_and_limits_are_those_of_the_library():
    assert (vz.max_dim(), vz.max_thickness(), vz.max_scale()) == (vz._MAX_DIM, vz._MAX_T, vz._MAX_SCALE)
    assert vz.GUARD > vz._MAX_T // 2 and 16 * vz._MAX_DIM + 2 * vz.GUARD < 2 ** 18
    before = dict(vz.PATHS)
    vz.render_cameras(**cases.camera_case("front"))
    assert vz.PATHS["torch"] == before["torch"] + 1 and vz.PATHS["kernel"] == before["kernel"]
    with pytest.raises(ValueError):
        vz.render_cameras(**dict(cases.camera_case("front"), thickness=200.0))
    with pytest.raises(ValueError):
        vz.render_cameras(**dict(cases.camera_case("front"), scale=0))


def test_tool_writes_pngs_equal_to_the_arrays(tmp_path):
    from PIL import Image
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import importlib
        tool = importlib.import_module("visualize")
    finally:
        sys.path.pop(0)
    out = str(tmp_path / "vis")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "visualize.py"), "--synthetic", "--small", "--frames", "2", "--scale", "2",
                        "--device", "cpu", "--out", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "mp4" in subprocess.run([sys.executable, os.path.join(ROOT, "tools", "visualize.py"), "--help"], capture_output=True,
                                   text=True).stdout
    tracker = vz.Tracker3D()
    for i, (meta, frames, points, pred) in enumerate(tool.synthetic_samples(2, small=True)):
        mosaic, bev = vz.visualize_sample(meta, frames, points, pred, tool.NUSC_CLASSES, tracker=tracker, scale=2)
        assert tuple(mosaic.shape) == (90, 240, 3) and tuple(bev.shape) == (1000, 1000, 3)
        assert (mosaic.numpy() != tiled(frames, scale=2)).any() and (bev.numpy() == 255).all(-1).any()
        assert np.array_equal(np.asarray(Image.open(os.path.join(out, "cameras", "%06d.png" % i))), mosaic.numpy())
        assert np.array_equal(np.asarray(Image.open(os.path.join(out, "bev", "%06d.png" % i))), bev.numpy())
