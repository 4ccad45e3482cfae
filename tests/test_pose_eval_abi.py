"""CPU-side checks of the pose-evaluation ABI (md2_pose_ate, csrc/traj.hip): struct layout,
every refusal and its message, workspace sizes — no kernel is launched — the host side of
pose_eval_ops and evaluate_pose, and the pin of the tests' numpy restatement
(tests/pose_eval_case.py) to the golden captured from the reference's own evaluate_pose.py."""
import ctypes

import numpy as np
import pytest
import torch  # noqa: F401  (load order: torch's HIP runtime first)

from monodepth2_amd import _lib
from monodepth2_amd.build import build
from monodepth2_amd.pose_eval_ops import check_offsets, pose_ate_desc, trajectory_ate

import pose_eval_case as pc

BAR_FACTOR = 8


@pytest.fixture(scope="module")
def L():
    build()
    return _lib.lib()


@pytest.fixture(scope="module")
def golden():
    return pc.load_golden()


def test_struct_layout_and_abi(L):
    D = _lib.PoseAteDesc
    assert ctypes.sizeof(D) == 32
    assert (D.sequences.offset, D.track_length.offset, D.flags.offset, D.reserved0.offset) == (0, 4, 8, 12)
    assert D.total_frames.offset == 16 and D.reserved.offset == 24
    assert L.md2_abi_version() == 24 == _lib.ABI_VERSION   # new symbols only: no bump
    assert {"md2_pose_ate", "md2_pose_ate_workspace_bytes"} <= set(_lib.EXPORTS)


BAD = [
    (dict(sequences=0), "sequences must be at least 1"),
    (dict(sequences=-3), "sequences must be at least 1"),
    (dict(track_length=1), "track_length must be 2..16"),
    (dict(track_length=0), "track_length must be 2..16"),
    (dict(track_length=17), "track_length must be 2..16"),
    (dict(sequences=3, total_frames=5), "2 * sequences"),
    (dict(sequences=1, total_frames=1), "2 * sequences"),
    (dict(sequences=1, total_frames=-4), "2 * sequences"),
    (dict(sequences=65536, total_frames=2 * 65536), "65535"),      # sequences are grid.y
    (dict(total_frames=2 ** 31), "too many frames"),
    (dict(total_frames=2 ** 40), "too many frames"),
]


def desc(**kw):
    args = dict(sequences=3, total_frames=1000, track_length=5)
    args.update(kw)
    return pose_ate_desc(**args)


def call(L, d, ptrs):
    return L.md2_pose_ate(ctypes.byref(d) if d is not None else None, *ptrs, None)


@pytest.mark.parametrize("kw,msg", BAD)
def test_invalid_desc_is_refused_with_a_message(L, kw, msg):
    d = desc(**kw)
    dummy = ctypes.c_void_p(256)   # non-NULL, never dereferenced: the desc is refused first
    assert L.md2_pose_ate_workspace_bytes(ctypes.byref(d)) == 0
    assert msg in L.md2_last_error().decode()
    assert call(L, d, [dummy] * 6) == -1
    assert msg in L.md2_last_error().decode()


def test_the_largest_legal_sizes_are_accepted(L):
    d = desc(sequences=65535, total_frames=2 ** 31 - 1, track_length=16)
    assert L.md2_pose_ate_workspace_bytes(ctypes.byref(d)) >= 96 * (2 ** 31 - 1 - 65535)
    assert L.md2_pose_ate_workspace_bytes(ctypes.byref(desc(sequences=1, total_frames=2, track_length=2))) == 256


def test_null_desc_and_operands(L):
    assert L.md2_pose_ate_workspace_bytes(None) == 0
    assert "NULL desc" in L.md2_last_error().decode()
    x = ctypes.c_void_p(256)
    assert call(L, None, [x] * 6) == -1
    assert "NULL desc" in L.md2_last_error().decode()
    d = desc()
    for hole in range(6):
        args = [x] * 6
        args[hole] = None
        assert call(L, d, args) == -1
        assert "NULL operand" in L.md2_last_error().decode()


def test_flags_and_misaligned_workspace(L):
    d = desc()
    d.flags = 1
    assert L.md2_pose_ate_workspace_bytes(ctypes.byref(d)) == 0
    assert "flags" in L.md2_last_error().decode()
    assert call(L, d, [ctypes.c_void_p(256)] * 6) == -1
    assert "flags" in L.md2_last_error().decode()
    d, x = desc(), ctypes.c_void_p(256)
    for off in (8, 16, 128):
        assert call(L, d, [x] * 5 + [ctypes.c_void_p(256 + off)]) == -1
        assert "256-byte aligned" in L.md2_last_error().decode()


def test_workspace_is_monotone_in_total_frames(L):
    sizes = []
    for frames in (6, 7, 8, 9, 300, 1591, 1591 + 1201, 10 ** 6):
        ws = L.md2_pose_ate_workspace_bytes(ctypes.byref(desc(total_frames=frames)))
        assert ws % 256 == 0 and ws >= 96 * (frames - 3)   # one 3x4 fp64 local pose per frame pair
        sizes.append(ws)
    assert all(a <= b for a, b in zip(sizes, sizes[1:])), sizes
    assert sizes[0] < sizes[-1]
    # the track length does not enter
    a = L.md2_pose_ate_workspace_bytes(ctypes.byref(desc(track_length=2)))
    assert a == L.md2_pose_ate_workspace_bytes(ctypes.byref(desc(track_length=16)))


def test_offsets_contract_is_checked_on_the_host_copy():
    check_offsets([0, 10], 10, 9)
    check_offsets([0, 2, 8, 10], 10, 7)
    for bad in ([1, 3, 10], [0, 5, 4, 10], [0, 3, 9], [0, 3, 11], [], [10]):
        with pytest.raises(ValueError, match="offsets"):
            check_offsets(bad, 10, 10 - max(len(bad) - 1, 0))
    for short in ([0, 1, 10], [0, 5, 5, 10], [0, 9, 10]):
        with pytest.raises(ValueError, match="at least 2 frames"):
            check_offsets(short, 10, 10 - (len(short) - 1))
    with pytest.raises(ValueError, match="7 predicted transforms"):
        check_offsets([0, 2, 8, 10], 10, 9)


def test_trajectory_ate_has_no_cpu_fallback():
    pred, gt = torch.zeros(5, 4, 4), torch.zeros(6, 3, 4, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="GPU only"):
        trajectory_ate(pred, gt)
    with pytest.raises(RuntimeError, match="GPU only"):
        trajectory_ate(pred, [gt])


def test_load_gt_poses_is_bit_equal_to_the_golden(golden, tmp_path):
    from monodepth2_amd.evaluate_pose import load_gt_poses
    for s, frames in enumerate(pc.FRAMES):
        path = tmp_path / ("%02d.txt" % s)
        path.write_text(str(golden["pose_text_%d" % s]))
        got, want = load_gt_poses(str(path)), golden["gt_%d" % s]
        assert got.dtype == np.float64 and got.shape == (frames, 3, 4)
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
        # the synthetic drive is regenerated identically (the GPU tests build other lengths from it)
        assert pc.drive_text(frames, pc.SEEDS[s]) == str(golden["pose_text_%d" % s])
        # six decimals: the rotations are orthonormal to ~1e-7, not to rounding
        R = want[:, :, :3]
        dev = np.abs(np.einsum("nij,nkj->nik", R, R) - np.eye(3)).max()
        assert 1e-8 < dev < 1e-5, dev


def worst(got, golden, s):
    want = np.concatenate([golden["ates_%d" % s], [golden["mean_%d" % s], golden["std_%d" % s]]])
    return float(np.max(np.abs(np.concatenate(got) - want) / np.abs(want)))


def test_golden_is_meaningful(golden):
    floor, rigid = float(golden["floor"]), float(golden["rigid"])
    assert 0 < floor < 1e-10 and rigid >= 100 * floor
    for s in range(len(pc.FRAMES)):
        a = golden["ates_%d" % s]
        assert a.shape == (pc.FRAMES[s] - 1,) and np.isfinite(a).all() and a.min() >= 1e-4
        assert str(golden["line_%d" % s]) == "\n   Trajectory error: {:0.3f}, std: {:0.3f}\n".format(
            float(golden["mean_%d" % s]), float(golden["std_%d" % s]))


@pytest.mark.parametrize("s", range(len(pc.FRAMES)))
def test_restatement_reproduces_the_reference_golden(golden, s):
    """The restatement (cofactor inverse, written order) against the reference's LAPACK
    inverses and np.dot chains.  The floor measured when the golden was made — the largest
    relative difference over all ATEs, means and stds — is 6.3e-12 (stored in the npz as
    `floor`): the conditioning of inverting poses ~560 m from the origin, ~1e-12 on
    translations of a metre, over errors of ~1e-2 m.  The bar is 8 x floor: the golden's
    host ran one BLAS/LAPACK, another reorders a handful of fp64 operations per inverse and
    product (an LU of a 4x4 and four-term dots: fewer than eight roundings apart)."""
    bar = BAR_FACTOR * float(golden["floor"])
    got = pc.trajectory_ate_np(golden["pred_poses_%d" % s], golden["gt_%d" % s])
    err = worst(got, golden, s)
    print("sequence", s, "restatement vs golden", err, "bar", bar)
    assert err <= bar


@pytest.mark.parametrize("s", range(len(pc.FRAMES)))
def test_rigid_inverse_misses_the_golden(golden, s):
    """[R^T | -R^T t] instead of the general inverse fails the same bar by orders of
    magnitude (1.2e-5 when the golden was made): the bar can see the shortcut."""
    bar = BAR_FACTOR * float(golden["floor"])
    got = pc.trajectory_ate_np(golden["pred_poses_%d" % s], golden["gt_%d" % s], inverse=pc.rigid_inverse)
    err = worst(got, golden, s)
    print("sequence", s, "rigid variant vs golden", err, "bar", bar)
    assert err > 100 * float(golden["floor"]) and err > bar


def test_cli_refuses_a_wrong_split_and_names_a_missing_file(tmp_path):
    from monodepth2_amd.evaluate_pose import evaluate
    from monodepth2_amd.options import MonodepthOptions
    parse = MonodepthOptions().parse
    with pytest.raises(SystemExit, match="eval_split should be either odom_9 or odom_10"):
        evaluate(parse(["--eval_split", "eigen", "--ext_poses_to_eval", str(tmp_path / "poses.npy")]))
    missing = str(tmp_path / "nowhere" / "09.txt")
    with pytest.raises(SystemExit, match="nowhere"):
        evaluate(parse(["--eval_split", "odom_9", "--ext_poses_to_eval", str(tmp_path / "poses.npy"),
                        "--gt_poses", missing]))
    # the default location: <data_path>/poses/NN.txt
    with pytest.raises(SystemExit, match="poses.10.txt"):
        evaluate(parse(["--eval_split", "odom_10", "--data_path", str(tmp_path),
                        "--ext_poses_to_eval", str(tmp_path / "poses.npy")]))
    (tmp_path / "09.txt").write_text("1 0 0 0 0 1 0 0 0 0 1 0\n1 0 0 0 0 1 0 0 0 0 1 1\n")
    with pytest.raises(SystemExit, match="poses.npy"):
        evaluate(parse(["--eval_split", "odom_9", "--ext_poses_to_eval", str(tmp_path / "poses.npy"),
                        "--gt_poses", str(tmp_path / "09.txt")]))
    with pytest.raises(NotImplementedError, match="out of scope"):
        evaluate(parse(["--eval_split", "odom_9", "--gt_poses", str(tmp_path / "09.txt")]))
