#!/usr/bin/env python3
"""Builds the ground-truth database ObjectSample reads (bevfusion_amd/gt_database.py) from a pickled list of `data_info` dicts.

    create_gt_database.py SAMPLES.pkl --data-path data/nuscenes --info-prefix nuscenes --classes car truck ... [--used-classes ...]

SAMPLES.pkl: what pickle.dump wrote of [dataset.get_data_info(j) for j in range(len(dataset))] on the stack that has the dataset
classes (sample_idx, lidar_points.lidar_path, lidar_sweeps, timestamp, ann_info with gt_bboxes_3d as a float32 array and
gt_labels_3d), or of a dict with the key `data_list` holding that list.  The pipeline is the reference's for NuScenesDataset
(LoadPointsFromFile 5/5, LoadPointsFromMultiSweeps with ten sweeps, LoadAnnotations3D); --no-defer merges the sweeps on the host.
Writes DATA_PATH/{prefix}_gt_database/*.bin and DATA_PATH/{prefix}_dbinfos_train.pkl."""
import argparse
import os
import pickle
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

import bevfusion_amd  # noqa: E402,F401
from bevfusion_amd import box_ops, gt_database  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("samples", help="pickled list of data_info dicts")
    ap.add_argument("--data-path", required=True)
    ap.add_argument("--info-prefix", required=True)
    ap.add_argument("--classes", nargs="+", required=True, help="label -> name, in label order (metainfo.classes)")
    ap.add_argument("--used-classes", nargs="+", default=None, help="classes that get an info entry (default: all)")
    ap.add_argument("--database-save-path", default=None)
    ap.add_argument("--db-info-save-path", default=None)
    ap.add_argument("--absolute-path", action="store_true", help="absolute file paths in the infos (relative_path=False)")
    ap.add_argument("--no-defer", action="store_true", help="merge the sweeps on the host instead of in the point kernels")
    ap.add_argument("--device", default=None, help="cuda:0, cpu, ... (default: the GPU when there is one)")
    args = ap.parse_args(argv)
    with open(args.samples, "rb") as f:
        samples = pickle.load(f)
    if isinstance(samples, dict):
        samples = samples["data_list"]
    infos = gt_database.create_groundtruth_database(
        samples, gt_database.nuscenes_pipeline(defer=not args.no_defer), args.classes, args.data_path, args.info_prefix,
        used_classes=args.used_classes, database_save_path=args.database_save_path, db_info_save_path=args.db_info_save_path,
        relative_path=not args.absolute_path, device=args.device)
    for name, entries in infos.items():
        print("load %d %s database infos" % (len(entries), name))
    print("points_in_boxes calls: %s" % (box_ops.PATHS,))


if __name__ == "__main__":
    main()
