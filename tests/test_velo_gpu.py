"""GPU tests of the velodyne projection operator (csrc/velo.hip, velo_ops.project_velodyne)
and of the layers above it: kitti_utils.generate_depth_map(s), the export_gt_depth command
line and device-resident ground truth in evaluate_depth.evaluate_disparities.

Yardsticks: the golden captured from the reference's own kitti_utils.generate_depth_map
(tests/golden/velo) and tests/velo_case.py, its numpy restatement (sort / ufunc.at), which
evaluates the projection in the kernel's written order.  Bars: against the restatement
everything is bitwise.  Against the golden the occupied pixels are identical, the values
bitwise with vel_depth (they are the input's fp32 x) and within 1 fp32 ulp without it: the
reference's np.dot goes through BLAS, so its summation order (and the last fp64 bit before
the fp32 rounding) may differ.  No valid golden point lies within 1e-9 of a rounding
boundary (checked when it was made and in test_velo_abi.py), so nothing is left out.
"""
import numpy as np
import pytest
import torch

import velo_case as vc
from monodepth2_amd.velo_ops import project_velodyne, workspace_bytes

pytestmark = pytest.mark.gpu

DEV = "cuda"


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run(frames, P, H, W, vel=False, **kw):
    """frames: list of (n, 4) fp32 arrays; P (B, 3, 4) -> (B, H, W) fp32 numpy."""
    out = project_velodyne([cuda(np.asarray(f, dtype=np.float32).reshape(-1, 4)) for f in frames], None,
                           cuda(np.asarray(P, dtype=np.float64)), H, W, vel_depth=vel, **kw)
    assert out.shape == (len(frames), H, W) and out.dtype == torch.float32 and out.is_cuda
    return out.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def restate(frames, P, H, W, vel=False):
    return np.stack([vc.depth_map_np(np.asarray(f, dtype=np.float32).reshape(-1, 4), p, H, W, vel)
                     for f, p in zip(frames, P)]).astype(np.float32)


def ulp_distance(a, b):
    """fp32 values of equal sign as ordered integers."""
    ia, ib = bits(a).astype(np.int64), bits(b).astype(np.int64)
    return np.abs(ia - ib)


@pytest.fixture(scope="module")
def golden():
    return vc.load_golden()


# 1 ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("vel", [False, True])
@pytest.mark.parametrize("cam", vc.CAMS)
def test_golden(golden, cam, vel):
    for scene, (H, W) in enumerate(vc.SIZES):
        pts, P = golden["points_%d" % scene], golden["P_%d_cam%d" % (scene, cam)]
        want = golden["depth_%d_cam%d_vel%d" % (scene, cam, int(vel))]
        got = run([pts], P[None], H, W, vel)[0]
        assert np.array_equal(got != 0, want != 0)
        dist = ulp_distance(got, want)
        print(f"scene {scene} cam {cam} vel_depth {vel}: {np.count_nonzero(want)} occupied, "
              f"{int((dist == 0).sum())} of {dist.size} bit-equal, {int((dist == 1).sum())} at 1 ulp, "
              f"max {int(dist.max())} ulp")
        assert (got >= 0).all()
        if vel:
            assert np.array_equal(bits(got), bits(want))
        else:
            assert dist.max() <= 1


# 2 ---------------------------------------------------------------------------------------

def small_P(H, W, seed):
    """A camera looking along +x over an H x W image, slightly rotated, so that the cloud
    of `small_scan` covers the frame and spills over every edge."""
    rng = np.random.default_rng(seed)
    f = 0.6 * W
    K = np.array([[f, 0, 0.5 * W + 0.5, 0], [0, f, 0.5 * H + 0.5, 0], [0, 0, 1, 0.0]])
    M = np.eye(4)
    M[:3, :3] = vc._rot(*rng.uniform(-0.03, 0.03, 3)) @ np.array([[0.0, -1, 0], [0, 0, -1], [1, 0, 0]])
    M[:3, 3] = [rng.uniform(-0.05, 0.05), rng.uniform(-0.05, 0.05), -0.3]
    return K @ M


def small_scan(n, H, W, seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.5, 30.0, n)
    y = x * rng.uniform(-1.1, 1.1, n)
    z = x * rng.uniform(-1.1, 1.1, n) * H / W
    x[rng.uniform(size=n) < 0.1] *= -1                    # behind the sensor
    near = rng.uniform(size=n) < 0.01                     # in front of the sensor, behind the camera
    x[near] = rng.uniform(0, 0.29, near.sum())
    y[near] *= 0.01
    z[near] *= 0.01
    return np.stack([x, y, z, rng.uniform(size=n)], 1).astype(np.float32)


@pytest.mark.parametrize("vel", [False, True])
@pytest.mark.parametrize("H,W", [(8, 8), (13, 41), (5, 2)])
def test_batch_against_the_restatement(H, W, vel):
    frames = [small_scan(40 * H * W, H, W, 1), np.zeros((0, 4), np.float32), small_scan(7 * H * W + 3, H, W, 2)]
    P = np.stack([small_P(H, W, s) for s in (5, 6, 7)])
    want = restate(frames, P, H, W, vel)
    got = run(frames, P, H, W, vel)
    assert np.count_nonzero(want[0]) > 0.5 * H * W and np.count_nonzero(want[2]) > 0
    assert not got[1].any() and np.array_equal(bits(got[1]), bits(want[1]))   # +0.0 everywhere
    assert np.array_equal(bits(got), bits(want)), np.argwhere(bits(got) != bits(want))[:10]
    # the quirk is in play: the maps are not the per-pixel minimum
    plain = np.stack([vc.pixel_min_np(f, p, H, W, vel) for f, p in zip(frames, P)]).astype(np.float32)
    assert (plain != want).any()


def test_offsets_tensor_form_and_many_frames():
    """The (points, offsets) form with offsets on the device, B = 70 frames of uneven sizes
    (several scatter blocks for the long ones, none for the empty ones)."""
    H, W = 13, 41
    rng = np.random.default_rng(0)
    sizes = rng.integers(0, 900, 70)
    sizes[3], sizes[10] = 0, 5000
    frames = [small_scan(int(n), H, W, 100 + i) for i, n in enumerate(sizes)]
    P = np.stack([small_P(H, W, 200 + i) for i in range(70)])
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    got = project_velodyne(cuda(np.concatenate(frames)), cuda(offsets), cuda(P), H, W).cpu().numpy()
    assert np.array_equal(bits(got), bits(restate(frames, P, H, W)))
    with pytest.raises(ValueError, match="offsets"):   # a host copy is checked
        project_velodyne(cuda(np.concatenate(frames)), torch.from_numpy(offsets[::-1].copy()), cuda(P), H, W)


# 3 ---------------------------------------------------------------------------------------

HALF_P = np.array([[0.0, 4, 0, 0], [0, 0, 4, 0], [1, 0, 0, 0]])   # u + 1 = rint(4 y), v + 1 = rint(4 z) at x = 1


def pt(y, z, x=1.0):
    return [x, y, z, 0.0]


def test_rounding_is_half_to_even_before_the_shift():
    H, W = 6, 6
    # 4 y = k / 2 for y = k / 8: exact half-integers; rint: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, 3.5 -> 4, 4.5 -> 4
    cases = [(1 / 8, None), (-1 / 8, None), (3 / 8, 1), (5 / 8, 1), (7 / 8, 3), (9 / 8, 3), (11 / 8, 5), (13 / 8, 5),
             (15 / 8, None)]   # 7.5 -> 8 -> column 7: off a 6-wide frame
    for k, (y, col) in enumerate(cases):
        depth = 2.0 + k
        for axis in (0, 1):     # the same along u and along v (the other coordinate lands on 2)
            p = pt(y, 3 / 4, depth) if axis == 0 else pt(3 / 4, y, depth)
            p[1] *= depth
            p[2] *= depth       # q0 / q2 = 4 y exactly: powers of two times a small integer
            got = run([[p]], HALF_P[None], H, W)[0]
            want = np.zeros((H, W), np.float32)
            if col is not None:
                want[(2, col) if axis == 0 else (col, 2)] = depth
            assert np.array_equal(bits(got), bits(want)), (y, axis, np.argwhere(got))
            assert np.array_equal(bits(got), bits(restate([[p]], HALF_P[None], H, W)[0]))


# 4 ---------------------------------------------------------------------------------------

def at(v, u, depth):
    """A point of HALF_P that lands on pixel (v, u) with the given depth."""
    return pt((u + 1) / 4 * depth, (v + 1) / 4 * depth, depth)


def wrap_case(points, H=4, W=5):
    got = run([points], HALF_P[None], H, W)[0]
    assert np.array_equal(bits(got), bits(restate([points], HALF_P[None], H, W)[0]))
    return got


def test_wrap_rule_first_point_takes_the_minimum_of_both_pixels():
    W = 5
    # first point on (1, W-1), the minimum on (2, 0): (1, W-1) gets 3, (2, 0) keeps its last write
    got = wrap_case([at(1, W - 1, 9), at(2, 0, 3), at(2, 0, 7), at(1, W - 1, 8)])
    assert got[1, W - 1] == 3 and got[2, 0] == 7 and np.count_nonzero(got) == 2
    # mirrored: first point on (2, 0), the minimum on (1, W-1)
    got = wrap_case([at(2, 0, 9), at(1, W - 1, 3), at(1, W - 1, 7), at(2, 0, 8)])
    assert got[2, 0] == 3 and got[1, W - 1] == 7 and np.count_nonzero(got) == 2
    # the first pixel's own points hold the minimum: the partner still keeps its last write, not its minimum
    got = wrap_case([at(1, W - 1, 2), at(2, 0, 5), at(2, 0, 4), at(2, 0, 6)])
    assert got[1, W - 1] == 2 and got[2, 0] == 6


def test_wrap_rule_pair_with_one_point_each():
    W = 5
    got = wrap_case([at(0, W - 1, 5), at(1, 0, 4)])
    assert got[0, W - 1] == 4 and got[1, 0] == 4        # the group's minimum, and the lone last write
    got = wrap_case([at(1, 0, 5), at(0, W - 1, 4)])
    assert got[1, 0] == 4 and got[0, W - 1] == 4
    got = wrap_case([at(1, 0, 4), at(0, W - 1, 5)])
    assert got[1, 0] == 4 and got[0, W - 1] == 5
    # (0, 0) and (H-1, W-1) have no partner; nor do columns in between
    got = wrap_case([at(0, 0, 5), at(3, W - 1, 4), at(0, 0, 6), at(2, 2, 9), at(2, 3, 1)])
    assert got[0, 0] == 5 and got[3, W - 1] == 4 and got[2, 2] == 9 and got[2, 3] == 1


def test_wrap_rule_three_rows_chained():
    W = 5
    # keys: {(0,W-1),(1,0)}, {(1,W-1),(2,0)}, {(2,W-1),(3,0)}; row 1 and 2 pixels belong to different groups
    pts = [at(1, 0, 8), at(0, W - 1, 2), at(1, W - 1, 6), at(2, 0, 1), at(2, 0, 5), at(3, 0, 7), at(2, W - 1, 9),
           at(2, W - 1, 3), at(1, 0, 4)]
    got = wrap_case(pts)
    assert got[1, 0] == 2          # first of its group: min(8, 2, 4)
    assert got[0, W - 1] == 2      # its only point
    assert got[1, W - 1] == 1      # first of its group: min(6, 1, 5)
    assert got[2, 0] == 5          # last write
    assert got[3, 0] == 3          # first of its group: min(7, 9, 3)
    assert got[2, W - 1] == 3      # last write
    assert np.count_nonzero(got) == 6


# 5 ---------------------------------------------------------------------------------------

def test_contention_and_order():
    """5000 points on one pixel and the same set permuted: the minimum does not move; the
    neighbour (2, 3) is in nobody's group, hit once per call, and follows the order."""
    H, W = 4, 5
    rng = np.random.default_rng(3)
    depths = rng.permutation(5000).astype(np.float64) / 16 + 1.0     # distinct, exact in fp32
    crowd = [at(2, 2, d) for d in depths]
    perm = rng.permutation(5000)
    a = crowd + [at(2, 3, 40.0)]
    b = [crowd[i] for i in perm] + [at(2, 3, 41.0)]
    ga, gb = wrap_case(a, H, W), wrap_case(b, H, W)
    assert ga[2, 2] == gb[2, 2] == 1.0
    assert ga[2, 3] == 40.0 and gb[2, 3] == 41.0
    # a wrapped pair under contention: the crowd on (1, W-1), one earlier point on (2, 0)
    c = [at(2, 0, 500.0)] + [at(1, W - 1, d) for d in depths] + [at(2, 0, 450.0)]
    gc = wrap_case(c, H, W)
    assert gc[2, 0] == 1.0 and gc[1, W - 1] == depths[-1]
    # last-writer order inside the crowd: reversing the points flips which value survives on the partner
    gd = wrap_case([at(2, 0, 500.0)] + [at(1, W - 1, d) for d in depths[::-1]], H, W)
    assert gd[2, 0] == 1.0 and gd[1, W - 1] == depths[0]


# 6 ---------------------------------------------------------------------------------------

def test_special_values():
    H, W = 4, 5
    nan, inf = float("nan"), float("inf")
    junk = [[nan, 1, 1, 0], [1, nan, 1, 0], [1, 1, nan, 0], [inf, 1, 1, 0], [1, inf, 1, 0], [1, -inf, 1, 0],
            [1, 1, inf, 0], [-inf, 1, 1, 0], [0.0, 1, 1, 0], [0.0, 0, 0, 0], [-1.0, 0.5, 0.5, 0],
            [1e-30, 1e30, 1e30, 0], [1, 1, 1, nan]]   # q2 == 0: 1/0, 0/0; the reflectance is ignored
    for vel in (False, True):
        got = run([junk], HALF_P[None], H, W, vel)[0]
        want = np.zeros((H, W), np.float32)
        want[3, 3] = 1.0      # only the last row is a point: (1, 1, 1) -> rint(4) - 1 = 3
        assert np.array_equal(bits(got), bits(want)), (vel, got)
        assert np.array_equal(bits(got), bits(restate([junk], HALF_P[None], H, W, vel)[0]))
    # x = -0.0 is kept (-0.0 >= 0); its camera depth comes from P, not from x
    P = np.array([[0.0, 4, 0, 0], [0, 0, 4, 0], [0, 0, 0, 1.0]])   # q2 = 1
    got = run([[[-0.0, 0.5, 0.75, 0]]], P[None], H, W)[0]
    assert got[2, 1] == 1.0 and np.count_nonzero(got) == 1
    got = run([[[-0.0, 0.5, 0.75, 0]]], P[None], H, W, True)[0]   # vel_depth: the map holds x = -0.0, not < 0
    assert np.array_equal(bits(got), bits(restate([[[-0.0, 0.5, 0.75, 0]]], P[None], H, W, True)[0]))
    assert not got.any()
    # negative camera depth: valid (both quotients positive), clamped to 0; a positive
    # point on the same pixel loses against it, as in the reference (the minimum is negative)
    N = np.array([[0.0, 4, 0, 0], [0, 0, 4, 0], [-1.0, 0, 0, 0]])   # q2 = -x
    neg = [[2.0, -1.0, -1.5, 0], [2.0, -1.0, -1.5, 0]]              # (-4 / -2, -6 / -2) -> pixel (2, 1), depth -2
    got = run([neg], N[None], H, W)[0]
    assert np.array_equal(bits(got), bits(np.zeros((H, W), np.float32)))
    tiny = [[1e-300, 0, 0, 0]]                                      # fp64 -1e-300... x is fp32: 0 -> q2 = -0.0
    assert np.array_equal(bits(run([tiny], N[None], H, W)[0]), bits(restate([tiny], N[None], H, W)[0]))
    # a negative fp64 depth that rounds to -0.0f, which is not < 0 in fp32: still 0, as +0.0
    s = 2.0 ** -100
    S = np.array([[0.0, 4 * s, 0, 0], [0, 0, 4 * s, 0], [-s, 0, 0, 0]])   # q2 = -2^-170 at x = 2^-70
    x = 2.0 ** -70
    small = [[x, -0.5 * x, -0.75 * x, 0]]
    for pts in (small, small + small):
        got = run([pts], S[None], H, W)[0]
        assert np.array_equal(bits(got), bits(restate([pts], S[None], H, W)[0])), got
    with_vel = run([neg + [[5.0, -2.5, -3.75, 0]]], N[None], H, W, True)[0]   # vel_depth: x itself, positive
    assert with_vel[2, 1] == 2.0 and np.count_nonzero(with_vel) == 1


# 7 ---------------------------------------------------------------------------------------

def test_workspace_reuse_leaves_no_stale_records():
    H, W = 13, 41
    A = [small_scan(3000, H, W, 11), small_scan(2000, H, W, 12)]
    B = [small_scan(4000, H, W, 13), small_scan(10, H, W, 14)]
    P = np.stack([small_P(H, W, 21), small_P(H, W, 22)])
    ws = torch.full((workspace_bytes(2, H, W, 5000),), 0xAB, dtype=torch.uint8, device=DEV)   # dirty on entry
    first = run(A, P, H, W, workspace=ws)
    other = run(B, P, H, W, workspace=ws)
    again = run(A, P, H, W, workspace=ws)
    assert np.array_equal(bits(first), bits(again))
    assert not np.array_equal(bits(first), bits(other))
    assert np.array_equal(bits(first), bits(restate(A, P, H, W)))
    with pytest.raises(ValueError, match="workspace"):
        run(A, P, H, W, workspace=ws[:1024])


def test_capturable_and_replay_follows_the_operands():
    """The chain in a captured graph: a replay after the points were rewritten in place
    gives the new scene's maps (memset, scatter and resolve are all in the graph)."""
    H, W = 13, 41
    A = [small_scan(3000, H, W, 31), small_scan(1000, H, W, 32)]
    B = [small_scan(3000, H, W, 33), small_scan(1000, H, W, 34)]     # same counts, other points
    P = np.stack([small_P(H, W, 41), small_P(H, W, 42)])
    pts, off, Pd = cuda(np.concatenate(A)), cuda(np.array([0, 3000, 4000], dtype=np.int64)), cuda(P)
    ws = torch.empty(workspace_bytes(2, H, W, 4000), dtype=torch.uint8, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = project_velodyne(pts, off, Pd, H, W, workspace=ws)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = project_velodyne(pts, off, Pd, H, W, workspace=ws)
    out.fill_(-1.0)
    graph.replay()
    first = out.clone()
    pts.copy_(cuda(np.concatenate(B)))
    graph.replay()
    second = out.clone()
    torch.cuda.synchronize()
    assert np.array_equal(bits(first.cpu().numpy()), bits(eager.cpu().numpy()))
    assert np.array_equal(bits(first.cpu().numpy()), bits(restate(A, P, H, W)))
    assert np.array_equal(bits(second.cpu().numpy()), bits(restate(B, P, H, W)))


# 8 ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def kitti_tree(golden, tmp_path_factory):
    """A KITTI-raw-like directory from the golden: two dates (rigs), one drive and one scan each."""
    root = tmp_path_factory.mktemp("kitti")
    lines, frames = [], []
    for scene in (0, 1):
        date = "2011_09_%02d" % (26 + scene)
        drive = "%s/%s_drive_0001_sync" % (date, date)
        vc.write_calib_dir(str(root / date), (str(golden["cam2cam_%d" % scene]), str(golden["velo2cam_%d" % scene])))
        data = root / drive / "velodyne_points" / "data"
        data.mkdir(parents=True)
        golden["points_%d" % scene].tofile(str(data / ("%010d.bin" % (7 + scene))))
        lines.append("%s %d l" % (drive, 7 + scene))
        frames.append((str(root / date), str(data / ("%010d.bin" % (7 + scene)))))
    return root, lines, frames


def test_generate_depth_map_and_export_cli(golden, kitti_tree, tmp_path):
    from monodepth2_amd import kitti_utils as ku
    from monodepth2_amd.export_gt_depth import export_gt_depths_kitti, parse_args
    root, lines, frames = kitti_tree
    for scene, (calib_dir, scan) in enumerate(frames):
        for cam in vc.CAMS:
            for vel in (False, True):
                got = ku.generate_depth_map(calib_dir, scan, cam, vel)
                want = golden["depth_%d_cam%d_vel%d" % (scene, cam, int(vel))]
                assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == want.shape
                assert np.array_equal(got != 0, want != 0)
                if vel:
                    assert np.array_equal(bits(got), bits(want))
                else:
                    assert ulp_distance(got, want).max() <= 1
    # the command line: frames of two sizes -> an object array; of one size -> a stacked array
    split = tmp_path / "test_files.txt"
    split.write_text("\n".join(lines) + "\n")
    out = export_gt_depths_kitti(parse_args(["--data_path", str(root), "--split", "eigen", "--split_file", str(split)]))
    assert out == str(tmp_path / "gt_depths.npz")
    data = np.load(out, fix_imports=True, encoding="latin1", allow_pickle=True)["data"]   # as evaluate_depth loads it
    assert data.dtype == object and len(data) == 2
    for scene in (0, 1):
        assert data[scene].dtype == np.float32
        assert np.array_equal(bits(data[scene]), bits(golden["depth_%d_cam2_vel1" % scene]))
    split.write_text("\n".join([lines[1]] * 3) + "\n")
    out = export_gt_depths_kitti(parse_args(["--data_path", str(root), "--split", "eigen", "--split_file", str(split),
                                             "--output", str(tmp_path / "same.npz"), "--batch_size", "2"]))
    data = np.load(out)["data"]
    assert data.dtype == np.float32 and data.shape == (3,) + vc.SIZES[1]
    assert all(np.array_equal(bits(d), bits(golden["depth_1_cam2_vel1"])) for d in data)


def test_device_ground_truth_equals_host_ground_truth(kitti_tree):
    """evaluate_disparities fed maps that never left the device, the same maps as host
    arrays, and evaluate_from_velodyne: bitwise the same results."""
    import types
    from monodepth2_amd import kitti_utils as ku
    from monodepth2_amd.evaluate_depth import evaluate_disparities, evaluate_from_velodyne
    _, _, frames = kitti_tree
    frames = [frames[1], frames[0], frames[1]]            # two sizes, grouped
    opt = types.SimpleNamespace(min_depth=0.1, max_depth=100.0, eval_split="eigen")
    rng = np.random.default_rng(5)
    disp = rng.uniform(0.02, 0.9, (3, 1, 24, 80)).astype(np.float32)
    dev = ku.generate_depth_maps(frames, cam=2, vel_depth=True)
    assert all(m.is_cuda and m.dtype == torch.float32 for m in dev)
    assert [tuple(m.shape) for m in dev] == [vc.SIZES[1], vc.SIZES[0], vc.SIZES[1]]
    on_device = evaluate_disparities(disp, dev, opt)
    on_host = evaluate_disparities(disp, [m.cpu().numpy() for m in dev], opt)
    chained = evaluate_from_velodyne(disp, frames, opt)
    same = torch.stack([dev[0], dev[2]])                  # the (N, GH, GW) tensor form
    stacked = evaluate_disparities(disp[[0, 2]], same, opt)
    assert (on_host["counts"] > 0).all()
    for key in ("errors", "ratios", "counts"):
        assert np.array_equal(on_device[key].view(np.uint64), on_host[key].view(np.uint64)), key
        assert np.array_equal(chained[key].view(np.uint64), on_host[key].view(np.uint64)), key
        assert np.array_equal(stacked[key].view(np.uint64), on_host[key][[0, 2]].view(np.uint64)), key
