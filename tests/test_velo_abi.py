"""CPU-side checks of the velodyne projection ABI (md2_velo_project, csrc/velo.hip): struct
layout, every refusal and its message, workspace sizes — no kernel is launched — the host
side of kitti_utils on the golden's calibration texts, the pin of the tests' numpy
restatement (tests/velo_case.py) to the golden captured from the reference's own
kitti_utils.generate_depth_map, and the export command line's missing-file error."""
import ctypes
import os

import numpy as np
import pytest
import torch  # noqa: F401  (load order: torch's HIP runtime first)

from monodepth2_amd import _lib
from monodepth2_amd.build import build
from monodepth2_amd.velo_ops import check_offsets, project_velodyne, velo_desc

import velo_case as vc


@pytest.fixture(scope="module")
def L():
    build()
    return _lib.lib()


def test_struct_layout_and_abi(L):
    assert ctypes.sizeof(_lib.VeloDesc) == 32
    D = _lib.VeloDesc
    assert (D.batch.offset, D.height.offset, D.width.offset, D.flags.offset) == (0, 4, 8, 12)
    assert D.total_points.offset == 16 and D.reserved.offset == 24
    assert _lib.VELO_VEL_DEPTH == 1
    assert L.md2_abi_version() == 24 == _lib.ABI_VERSION   # new symbols only: no bump
    assert {"md2_velo_project", "md2_velo_project_workspace_bytes"} <= set(_lib.EXPORTS)


BAD = [
    (dict(batch=0), "positive"),
    (dict(batch=-1), "positive"),
    (dict(height=0), "positive"),
    (dict(width=0), "positive"),
    (dict(width=-5), "positive"),
    (dict(total_points=0), "positive"),
    (dict(total_points=-7), "positive"),
    (dict(width=1), "width must be at least 2"),
    (dict(batch=65536, height=2, width=2), "65535"),              # frames are grid.y
    (dict(batch=4611, height=375, width=1242), "2^31 pixels"),
    (dict(batch=1, height=1, width=2 ** 31 - 1), "2^31 pixels"),
    (dict(batch=2, height=2 ** 15, width=2 ** 15), "2^31 pixels"),
    (dict(total_points=2 ** 31), "too many points"),
    (dict(total_points=2 ** 40), "too many points"),
]


def desc(**kw):
    args = dict(batch=3, height=13, width=41, total_points=1000)
    args.update(kw)
    return velo_desc(**args)


@pytest.mark.parametrize("kw,msg", BAD)
def test_invalid_desc_is_refused_with_a_message(L, kw, msg):
    d = desc(**kw)
    dummy = ctypes.c_void_p(256)   # non-NULL, never dereferenced: the desc is refused first
    assert L.md2_velo_project_workspace_bytes(ctypes.byref(d)) == 0
    assert msg in L.md2_last_error().decode()
    assert L.md2_velo_project(ctypes.byref(d), dummy, dummy, dummy, dummy, dummy, None) == -1
    assert msg in L.md2_last_error().decode()


def test_the_largest_legal_sizes_are_accepted(L):
    d = desc(batch=65535, height=2, width=2, total_points=2 ** 31 - 1)
    assert L.md2_velo_project_workspace_bytes(ctypes.byref(d)) >= 16 * 65535 * 4


def test_null_desc_and_operands(L):
    assert L.md2_velo_project_workspace_bytes(None) == 0
    assert "NULL" in L.md2_last_error().decode()
    x = ctypes.c_void_p(256)
    assert L.md2_velo_project(None, x, x, x, x, x, None) == -1
    assert "NULL" in L.md2_last_error().decode()
    d = desc()
    for hole in range(5):
        args = [x] * 5
        args[hole] = None
        assert L.md2_velo_project(ctypes.byref(d), *args, None) == -1
        assert "NULL operand" in L.md2_last_error().decode()


def test_unknown_flags_and_misaligned_workspace(L):
    d = desc()
    d.flags = 1 << 7
    assert L.md2_velo_project_workspace_bytes(ctypes.byref(d)) == 0
    assert "flags" in L.md2_last_error().decode()
    d, x = desc(), ctypes.c_void_p(256)
    assert L.md2_velo_project(ctypes.byref(d), x, x, x, x, ctypes.c_void_p(264), None) == -1
    assert "aligned" in L.md2_last_error().decode()


def test_workspace_is_monotone_in_pixels(L):
    sizes = []
    for B, H, W in [(1, 1, 2), (1, 5, 2), (1, 13, 41), (1, 37, 124), (3, 37, 124), (2, 375, 1242), (16, 375, 1242)]:
        ws = L.md2_velo_project_workspace_bytes(ctypes.byref(desc(batch=B, height=H, width=W)))
        assert ws % 256 == 0 and ws >= 16 * B * H * W   # one 16-byte record per pixel
        sizes.append((B * H * W, ws))
    assert all(a[1] <= b[1] for a, b in zip(sizes, sizes[1:])), sizes
    assert sizes[0][1] < sizes[-1][1]
    # the points do not enter: they are read in place
    a = L.md2_velo_project_workspace_bytes(ctypes.byref(desc(total_points=1)))
    assert a == L.md2_velo_project_workspace_bytes(ctypes.byref(desc(total_points=10 ** 9)))


def test_project_velodyne_has_no_cpu_fallback():
    P = torch.zeros(1, 3, 4, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="GPU only"):
        project_velodyne(torch.zeros(5, 4), torch.tensor([0, 5]), P, 8, 8)
    with pytest.raises(RuntimeError, match="GPU only"):
        project_velodyne([torch.zeros(5, 4)], None, P, 8, 8)


def test_offsets_contract_is_checked_on_the_host_copy():
    check_offsets([0, 3, 3, 10], 10)
    for bad in ([1, 3, 10], [0, 5, 4, 10], [0, 3, 9], [0, 3, 11], []):
        with pytest.raises(ValueError, match="offsets"):
            check_offsets(bad, 10)


@pytest.fixture(scope="module")
def golden():
    return vc.load_golden()


@pytest.mark.parametrize("scene", [0, 1])
def test_calibration_readers_match_the_reference(golden, scene, tmp_path):
    """read_calib_file on the golden's calibration texts against what the reference's reader
    made of them, and velo_to_image_matrix against the reference's np.dot chain on those
    recorded inputs, evaluated here: bit-equal.  Against the matrix recorded on the
    golden's host only up to the rounding of two chained four-term fp64 dots, whose order
    and fusing belong to the host's BLAS: |dP| <= 16 eps |P_rect| |R_rect| |velo2cam|
    (2 x gamma_4 = 8 eps, doubled)."""
    from monodepth2_amd import kitti_utils as ku
    cdir = vc.write_calib_dir(str(tmp_path / "rig"), (str(golden["cam2cam_%d" % scene]),
                                                      str(golden["velo2cam_%d" % scene])))
    cam2cam = ku.read_calib_file(os.path.join(cdir, "calib_cam_to_cam.txt"))
    velo = ku.read_calib_file(os.path.join(cdir, "calib_velo_to_cam.txt"))
    assert isinstance(cam2cam["calib_time"], str) and cam2cam["calib_time"] == "09-Jan-2012 13:57:47"
    for k in ("S_rect_02", "R_rect_00", "P_rect_02", "P_rect_03"):
        want = golden["calib_%d_%s" % (scene, k)]
        assert cam2cam[k].dtype == np.float64 and np.array_equal(cam2cam[k].view(np.uint64), want.view(np.uint64)), k
    for k in ("R", "T"):
        want = golden["calib_%d_%s" % (scene, k)]
        assert np.array_equal(velo[k].view(np.uint64), want.view(np.uint64)), k
    v2c = np.eye(4)
    v2c[:3, :3], v2c[:3, 3] = golden["calib_%d_R" % scene].reshape(3, 3), golden["calib_%d_T" % scene]
    rect = np.eye(4)
    rect[:3, :3] = golden["calib_%d_R_rect_00" % scene].reshape(3, 3)
    for cam in vc.CAMS:
        P, size = ku.velo_to_image_matrix(cdir, cam)
        proj = golden["calib_%d_P_rect_0%d" % (scene, cam)].reshape(3, 4)
        here = np.dot(np.dot(proj, rect), v2c)
        assert size == vc.SIZES[scene]
        assert P.dtype == np.float64 and P.shape == (3, 4)
        assert np.array_equal(P.view(np.uint64), here.view(np.uint64)), (cam, P - here)
        recorded = golden["P_%d_cam%d" % (scene, cam)]
        bound = 16 * np.finfo(np.float64).eps * (np.abs(proj) @ np.abs(rect) @ np.abs(v2c))
        print("cam", cam, "max |dP| / bound", (np.abs(P - recorded) / bound).max())
        assert (np.abs(P - recorded) <= bound).all()


def test_load_velodyne_points(tmp_path):
    from monodepth2_amd import kitti_utils as ku
    pts = vc.make_scan(50, seed=1)
    path = str(tmp_path / "scan.bin")
    pts.tofile(path)
    got = ku.load_velodyne_points(path)
    assert got.dtype == np.float32 and got.shape == (50, 4)
    assert np.array_equal(got[:, :3], pts[:, :3]) and (got[:, 3] == 1).all()


@pytest.mark.parametrize("scene", [0, 1])
@pytest.mark.parametrize("cam", vc.CAMS)
@pytest.mark.parametrize("vel", [False, True])
def test_restatement_reproduces_the_reference_golden(golden, scene, cam, vel):
    """Bitwise after the fp32 cast.  The restatement sums the projection in the written
    order, the reference through np.dot: they can differ in the last fp64 bit, which the
    fp32 cast absorbs on this data (checked when the golden was made), and no valid point
    is within 1e-9 of a rounding boundary, so no point changes pixel."""
    H, W = vc.SIZES[scene]
    pts, P = golden["points_%d" % scene], golden["P_%d_cam%d" % (scene, cam)]
    assert vc.half_integer_margin(pts, P, H, W) > 1e-9
    got = vc.depth_map_np(pts, P, H, W, vel).astype(np.float32)
    want = golden["depth_%d_cam%d_vel%d" % (scene, cam, int(vel))]
    assert want.dtype == np.float32 and want.shape == (H, W)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # the golden exercises the sub2ind quirk: it is not the plain per-pixel minimum
    plain = vc.pixel_min_np(pts, P, H, W, vel).astype(np.float32)
    cols = set(np.argwhere(plain != want)[:, 1].tolist())
    assert cols and cols <= {0, W - 1}


def test_export_cli_names_the_missing_split_file(tmp_path):
    from monodepth2_amd.export_gt_depth import export_gt_depths_kitti, parse_args
    missing = str(tmp_path / "nowhere" / "test_files.txt")
    with pytest.raises(SystemExit, match="nowhere"):
        export_gt_depths_kitti(parse_args(["--data_path", str(tmp_path), "--split", "eigen", "--split_file", missing]))
    # the default location: the tree ships no split lists
    with pytest.raises(SystemExit, match="test_files.txt"):
        export_gt_depths_kitti(parse_args(["--data_path", str(tmp_path), "--split", "eigen_benchmark"]))


def test_export_eigen_benchmark_reads_the_pngs_on_the_host(tmp_path):
    """The improved ground truth: 16-bit PNG / 256 (export_gt_depth.py:50-53), no GPU."""
    import PIL.Image as pil
    from monodepth2_amd.export_gt_depth import export_gt_depths_kitti, parse_args
    rng = np.random.default_rng(0)
    drive = "2011_09_26/2011_09_26_drive_0002_sync"
    folder = tmp_path / drive / "proj_depth" / "groundtruth" / "image_02"
    folder.mkdir(parents=True)
    maps = []
    for frame in (5, 69):
        raw = (rng.integers(0, 2 ** 16, (6, 9)) * (rng.uniform(size=(6, 9)) < 0.3)).astype(np.uint16)
        pil.fromarray(raw).save(str(folder / ("%010d.png" % frame)))
        maps.append(raw.astype(np.float32) / 256)
    split = tmp_path / "test_files.txt"
    split.write_text("%s 5 l\n%s 69 r\n" % (drive, drive))
    out = export_gt_depths_kitti(parse_args(["--data_path", str(tmp_path), "--split", "eigen_benchmark",
                                             "--split_file", str(split)]))
    data = np.load(out)["data"]
    assert data.dtype == np.float32 and np.array_equal(data, np.stack(maps))
    split.write_text("%s 6 l\n" % drive)
    with pytest.raises(SystemExit, match="0000000006.png"):
        export_gt_depths_kitti(parse_args(["--data_path", str(tmp_path), "--split", "eigen_benchmark",
                                           "--split_file", str(split)]))
