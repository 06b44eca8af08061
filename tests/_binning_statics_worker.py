"""Child process of tests/test_gpu_binning.py::test_library_statics_in_a_fresh_process.  The parent sets
GOL_SORT_BIG_NO_LDS=1 GOL_BIN_WGS=1 GOL_BIN_WGS2=1 (statics of the library, read on the first gol_bin_sort call): the BIG
kernel sorts on global memory, and both Gaussian walks use their largest chunk (4096 per workgroup).  Exits on the first
failure."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import binning_cases as bc  # noqa: E402
import test_gpu_binning as tb  # noqa: E402


def main():
    assert all(os.environ.get(k) == "1" for k in ("GOL_SORT_BIG_NO_LDS", "GOL_BIN_WGS", "GOL_BIN_WGS2"))
    # scenario (b): queues overflowing, BIG lists without their LDS
    scene, ids, bins = tb.planned("b")
    tb.assert_exact(tb.run_hip([scene], scene[3], scene[4], ids.numel()), 0, ids, bins)
    print("scenario b ok", flush=True)
    # N = 9096 = three scatter workgroups of 4096; the first one counts 4096 in both tiles
    scene = bc.two_tile_chunk_scene()
    xys, depths, radii, H, W, plan = scene
    ids, bins = bc.oracle_lists(xys, depths, radii, H, W)
    assert (bins[:, 1] - bins[:, 0]).tolist() == [plan[0], plan[1]]
    tb.assert_exact(tb.run_hip([scene], H, W, ids.numel()), 0, ids, bins)
    print("two-tile chunk scene ok", flush=True)
    # the pruning contract with one workgroup per walk
    for seed in (0, 1):
        scene, (ids, bins), live = tb.prune_case(seed)
        H, W = scene[5], scene[6]
        ws = tb.run_hip([scene], H, W, ids.numel(), pruned=True)
        tb.check_pruned(ws, 0, scene[0].shape[0], ids, bins, live, ids.numel())
    print("prune_scene ok", flush=True)
    print("BINNING_STATICS_OK")


if __name__ == "__main__":
    main()
