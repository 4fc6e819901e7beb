"""The recorded run of the reference's create_groundtruth_database (tests/golden/gt_database.npz, written by
tests/golden/make_gt_database_golden.py) as inputs and expectations for the CPU and GPU tests."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gt_database.npz")
_cache = {}


def golden():
    if "g" not in _cache:
        _cache["g"] = dict(np.load(GOLDEN))
    return _cache["g"]


def n_frames():
    return int(golden()["n_frames"])


def classes():
    return [str(c) for c in golden()["classes"]]


def used_classes():
    return [str(c) for c in golden()["used_classes"]]


def prefix():
    return str(golden()["info_prefix"])


def frame(f):
    """(points [n, C], boxes [K, 7 or 9], the reference's mask [n, K])."""
    g = golden()
    return g["frame%d_points" % f], g["frame%d_gt_bboxes_3d" % f], g["frame%d_mask" % f]


def samples():
    """The frames as data_info dicts with the points already loaded (fresh copies)."""
    g, out = golden(), []
    for f in range(n_frames()):
        key = "frame%d_" % f
        ann = {k: g[key + k].copy() for k in ("gt_bboxes_3d", "gt_labels_3d", "group_ids", "difficulty", "score") if key + k in g}
        out.append(dict(sample_idx=int(g[key + "sample_idx"]), points=g[key + "points"].copy(), ann_info=ann))
    return out


def files():
    """{file name: its bytes (uint8 array)} as the reference wrote them."""
    g = golden()
    ends = np.cumsum(g["file_sizes"])
    return {str(name): g["file_bytes"][end - size:end] for name, size, end in zip(g["file_names"], g["file_sizes"], ends)}


def frame_rows(f):
    """(counts [K], centred rows [sum, C]) of frame f as the reference's files hold them."""
    g, written = golden(), files()
    _, boxes, _ = frame(f)
    C = g["frame%d_points" % f].shape[1]
    names = [classes()[int(i)] for i in g["frame%d_gt_labels_3d" % f]]
    blobs = [written["%d_%s_%d.bin" % (int(g["frame%d_sample_idx" % f]), names[i], i)].view(np.float32).reshape(-1, C)
             for i in range(len(boxes))]
    return np.array([len(b) for b in blobs], np.int32), np.concatenate(blobs, 0)


def infos():
    """The reference's pickle: {class: [dict]} in its key and list order."""
    g, out, at, box_at = golden(), {}, 0, 0
    for name, size in zip(g["info_classes"], g["info_class_sizes"]):
        entries = []
        for _ in range(int(size)):
            cols = int(g["info_box_cols"][at])
            info = dict(name=str(g["info_name"][at]), path=str(g["info_path"][at]), image_idx=int(g["info_image_idx"][at]),
                        gt_idx=int(g["info_gt_idx"][at]), box3d_lidar=g["info_boxes"][box_at:box_at + cols],
                        num_points_in_gt=int(g["info_num_points_in_gt"][at]),
                        difficulty=np.dtype(str(g["info_difficulty_dtype"][at])).type(g["info_difficulty"][at]),
                        group_id=int(g["info_group_id"][at]))
            if not np.isnan(g["info_score"][at]):
                info["score"] = float(g["info_score"][at])
            entries.append(info)
            at, box_at = at + 1, box_at + cols
        out[str(name)] = entries
    return out


def same_infos(got, want):
    """Field by field; the dtype of box3d_lidar and of difficulty included."""
    assert list(got) == list(want), (list(got), list(want))
    for name in want:
        assert len(got[name]) == len(want[name]), name
        for a, b in zip(got[name], want[name]):
            assert sorted(a) == sorted(b), (sorted(a), sorted(b))
            for field in b:
                if field == "box3d_lidar":
                    assert a[field].dtype == np.float32 == b[field].dtype and a[field].shape == b[field].shape
                    assert np.array_equal(a[field].view(np.int32), b[field].view(np.int32)), (name, a["gt_idx"])
                elif field == "difficulty":
                    assert np.asarray(a[field]).dtype == np.asarray(b[field]).dtype and a[field] == b[field]
                else:
                    assert type(a[field]) in (type(b[field]), np.float64) and a[field] == b[field], (name, field, a[field], b[field])


def same_database(root, want_files=None):
    """The files under root/<prefix>_gt_database are the recorded ones, byte for byte, and no others."""
    want_files = files() if want_files is None else want_files
    db = os.path.join(root, prefix() + "_gt_database")
    assert sorted(os.listdir(db)) == sorted(want_files)
    for name, blob in want_files.items():
        assert np.array_equal(np.fromfile(os.path.join(db, name), dtype=np.uint8), blob), name
