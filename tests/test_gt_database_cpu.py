"""CPU: box_ops.torch_points_in_boxes / points_in_rbbox and gt_database.create_groundtruth_database(device="cpu") against the
recorded run of the reference's own builder (tests/golden/gt_database.npz), bit for bit; the database it writes feeds this
package's DataBaseSampler and ObjectSample."""
import os
import pickle

import numpy as np
import pytest
import torch

import gt_database_cases as cases
from bevfusion_amd import box_ops, gt_database
from bevfusion_amd.registry import TRANSFORMS


@pytest.mark.parametrize("f", range(4))
def test_specification_equals_the_reference_bit_for_bit(f):
    assert cases.n_frames() == 4
    points, boxes, mask = cases.frame(f)
    want_counts, want_rows = cases.frame_rows(f)
    counts, rows, got_mask = box_ops.torch_points_in_boxes(points, boxes, center=True, return_mask=True)
    assert counts.dtype == torch.int32 and np.array_equal(counts.numpy(), want_counts)
    assert np.array_equal(got_mask.numpy(), mask) and np.array_equal(mask.sum(0), want_counts)
    assert rows.dtype == torch.float32 and rows.shape == want_rows.shape
    assert np.array_equal(rows.numpy().view(np.int32), want_rows.view(np.int32))
    rb = box_ops.points_in_rbbox(points, boxes)
    assert isinstance(rb, np.ndarray) and rb.dtype == np.bool_ and np.array_equal(rb, mask)
    assert torch.equal(box_ops.points_in_rbbox(torch.from_numpy(points), boxes), torch.from_numpy(mask))
    # not centred: the member rows themselves, box-major, ascending point index
    counts2, plain = box_ops.torch_points_in_boxes(torch.from_numpy(points), boxes)
    want_plain = np.concatenate([points[mask[:, j]] for j in range(mask.shape[1])], 0)
    assert torch.equal(counts2, counts) and np.array_equal(plain.numpy().view(np.int32), want_plain.view(np.int32))


def test_the_fixture_holds_the_cases_it_claims():
    shared = nan_rows = 0
    for f in range(cases.n_frames()):
        points, boxes, mask = cases.frame(f)
        finite = np.isfinite(points[:, 0])
        shared += int((mask[finite].sum(1) > 1).sum())
        nan_rows += int((~finite).sum())
        assert mask[~finite].all() and not mask[finite, -1].any()       # a NaN row is in every box; the last box holds nothing else
    assert shared > 0 and nan_rows == 1
    assert {cases.frame(f)[1].shape[1] for f in range(4)} == {7, 9} and {cases.frame(f)[0].shape[1] for f in range(4)} == {3, 5}


def test_degenerate_inputs():
    pts = torch.zeros((5, 4))
    counts, rows = box_ops.torch_points_in_boxes(pts, np.zeros((0, 7), np.float32), center=True)
    assert counts.shape == (0,) and counts.dtype == torch.int32 and rows.shape == (0, 4)
    boxes = np.array([[0, 0, -1, 2, 2, 2, 0.3], [0, 0, -1, 0, 2, 2, 0.3]], np.float32)  # the second has a zero dimension
    counts, rows = box_ops.torch_points_in_boxes(pts, boxes)
    assert counts.tolist() == [5, 0] and rows.shape == (5, 4)
    counts, rows = box_ops.torch_points_in_boxes(torch.zeros((0, 3)), boxes, center=True)
    assert counts.tolist() == [0, 0] and rows.shape == (0, 3)
    with pytest.raises(ValueError):
        box_ops.torch_points_in_boxes(pts, np.zeros((2, 6), np.float32))


def _build(root, **kwargs):
    return gt_database.create_groundtruth_database(cases.samples(), [dict(type="LoadAnnotations3D")], cases.classes(), str(root),
                                                   cases.prefix(), used_classes=cases.used_classes(), device="cpu", **kwargs)


def test_builder_writes_the_reference_files_and_pickle(tmp_path):
    before = dict(box_ops.PATHS)
    returned = _build(tmp_path)
    assert box_ops.PATHS["torch"] == before["torch"] + cases.n_frames() and box_ops.PATHS["kernel"] == before["kernel"]
    cases.same_database(str(tmp_path))
    with open(os.path.join(str(tmp_path), cases.prefix() + "_dbinfos_train.pkl"), "rb") as fh:
        got = pickle.load(fh)
    want = cases.infos()
    cases.same_infos(got, want)
    cases.same_infos(returned, want)
    # files for the class left out, but no infos
    left_out = set(cases.classes()) - set(cases.used_classes())
    assert left_out == {"barrier"} and not left_out & set(got)
    assert any("_barrier_" in name for name in os.listdir(os.path.join(str(tmp_path), cases.prefix() + "_gt_database")))
    assert all(info["path"] == os.path.join(cases.prefix() + "_gt_database", "%d_%s_%d.bin" % (info["image_idx"], name, info["gt_idx"]))
               for name in got for info in got[name])
    # the running group counter: frame 0's repeated group_ids share an id, later frames count on
    ids = sorted(info["group_id"] for name in got for info in got[name])
    assert ids[0] == 0 and len(set(ids)) < len(ids) and ids[-1] == len(set(ids)) - 1


def test_builder_paths_and_defaults(tmp_path):
    db, pkl = tmp_path / "elsewhere", tmp_path / "infos.pkl"
    got = _build(tmp_path, database_save_path=str(db), db_info_save_path=str(pkl), relative_path=False)
    assert pkl.exists() and not (tmp_path / (cases.prefix() + "_gt_database")).exists()
    for name in got:
        for info in got[name]:
            assert os.path.isabs(info["path"]) and os.path.exists(info["path"])
    everything = gt_database.create_groundtruth_database(cases.samples(), [TRANSFORMS.build(dict(type="LoadAnnotations3D"))],
                                                         cases.classes(), str(tmp_path), "all", device="cpu")
    assert sorted(everything) == sorted(cases.classes()) and sum(len(v) for v in everything.values()) == len(cases.files())

    class Dataset:  # an object with __len__ and get_data_info instead of a list
        def __len__(self):
            return cases.n_frames()

        def get_data_info(self, j):
            return cases.samples()[j]

    again = gt_database.create_groundtruth_database(Dataset(), [dict(type="LoadAnnotations3D")], cases.classes(), str(tmp_path / "obj"),
                                                    cases.prefix(), used_classes=cases.used_classes(), device="cpu")
    cases.same_infos(again, cases.infos())


def test_with_mask_raises(tmp_path):
    with pytest.raises(NotImplementedError, match="with_mask"):
        _build(tmp_path, with_mask=True)


def test_database_feeds_the_sampler_and_object_sample(tmp_path):
    _build(tmp_path)
    used = cases.used_classes()
    cfg = dict(data_root=str(tmp_path), info_path=os.path.join(str(tmp_path), cases.prefix() + "_dbinfos_train.pkl"), rate=1.0,
               prepare=dict(filter_by_difficulty=[-1], filter_by_min_points={name: 3 for name in used}), classes=cases.classes(),
               sample_groups={name: 3 for name in used},
               points_loader=dict(type="LoadPointsFromFile", coord_type="LIDAR", load_dim=5, use_dim=[0, 1, 2, 3, 4]))
    with open(cfg["info_path"], "rb") as fh:
        infos = pickle.load(fh)  # what the builder wrote
    infos = {name: [i for i in infos[name] if i["image_idx"] in (100, 114)] for name in infos}  # 7-column boxes, 5 floats per point
    with open(cfg["info_path"], "wb") as fh:
        pickle.dump(infos, fh)
    np.random.seed(3)
    transform = TRANSFORMS.build(dict(type="ObjectSample", db_sampler=cfg))
    sampler = transform.db_sampler
    info = infos["car"][0]
    loaded = sampler.load_points(info)
    assert loaded.shape == (info["num_points_in_gt"], 5)
    points, boxes, _ = cases.frame(0)
    far = np.array([[60.0, 60.0, -1.0, 1.0, 1.0, 1.0, 0.0]], np.float32)
    data = dict(points=torch.from_numpy(points.copy()), gt_bboxes_3d=far, gt_labels_3d=np.array([0], np.int64))
    out = transform(data)
    pasted = len(out["gt_bboxes_3d"]) - 1
    assert pasted > 0 and len(out["gt_labels_3d"]) == pasted + 1
    # the pasted objects' points lie inside their boxes again
    new_boxes = np.ascontiguousarray(out["gt_bboxes_3d"][1:, :7])
    inside = box_ops.points_in_rbbox(out["points"][:, :5].contiguous(), new_boxes)
    assert int(inside.any(1).sum()) >= 3 * pasted  # filter_by_min_points left objects of three points or more
