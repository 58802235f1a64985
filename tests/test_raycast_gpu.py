"""hive_tsdf_raycast (csrc/raycast.hip) through ``TSDFVolume.raycast`` against the numpy restatement (tests/raycast_restatement.py): depth, vertex and normal
bits and the colours, at image sizes that leave wave and workgroup tiles partly empty, in a cubic and an odd volume, from poses that take every branch."""
import numpy as np
import pytest

import raycast_restatement as rc
import tracking_cases as tc

pytestmark = pytest.mark.gpu

IMAGES = [(1, 1), (5, 7), (24, 32), (47, 63), (48, 64)]
VOXEL = 0.05
VOLUMES = {"cube32": np.array([[0.0, 1.6]] * 3), "odd33x31x35": np.array([[0.0, 1.63], [0.0, 1.53], [0.0, 1.73]])}
FUSE_SIZE = (48, 64)


def _fused(oracle, bounds, poses):
    vol = oracle.TSDFVolume(bounds, VOXEL)
    K = tc.intrinsics(*FUSE_SIZE)
    for i, pose in enumerate(poses):
        color, depth = tc.room_frame(pose, K, *FUSE_SIZE, seed=i)
        vol.integrate(color, depth, K, pose)
    return vol


@pytest.fixture(scope="module")
def volumes(gpu_ctx, oracle_lib):
    """name -> (oracle volume, the same planes in a device volume): two orbit frames fused, and for "one side" a single frame."""
    from hive_amd import fusion
    orbit = tc.corner_orbit(12)
    out = {}
    for name, bounds in VOLUMES.items():
        for kind, poses in (("", orbit[:2]), ("/one side", orbit[:1])):
            ora = _fused(oracle_lib, bounds, poses)
            dev = fusion.TSDFVolume(bounds, VOXEL, ctx=gpu_ctx)
            assert tuple(dev.vol_dim) == ora._tsdf.shape
            dev.set_volume(ora._tsdf, ora._color, ora._weight)
            out[name + kind] = (ora, dev)
    assert out["cube32"][0]._tsdf.shape == (32, 32, 32) and out["odd33x31x35"][0]._tsdf.shape == (33, 31, 35)
    return out


# name -> (volume kind, pose, whole-pixel principal point, extra arguments)
CASES = {
    "corner": ("", tc.corner_orbit(12)[0], False, {}),
    "outside looking in": ("", tc.outside_pose(), False, {}),
    "looking away": ("", tc.away_pose(), False, {}),
    "axis-parallel rays": ("", tc.axis_pose(), True, {}),
    "one side, from behind the walls": ("/one side", tc.look_at([1.58, 0.9, 1.57], [0.6, 1.0, 0.65]), False, {}),
    "z_near and z_far": ("", tc.corner_orbit(12)[0], False, {"z_near": 0.9, "z_far": 1.15}),
    "coarse step": ("", tc.corner_orbit(12)[3], False, {"step": 0.9}),
}


def _restated(ora, K, pose, size, extra, stats=None):
    kw = {("step_in_trunc" if k == "step" else k): v for k, v in extra.items()}
    return rc.raycast(ora._tsdf, ora._weight, ora._color, ora._vol_origin, np.float32(ora._voxel_size), np.float32(ora._trunc_margin), size[0], size[1], K, pose,
                      stats=stats, **kw)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("volume", list(VOLUMES))
@pytest.mark.parametrize("case", list(CASES))
def test_raycast_matches_the_restatement_bit_for_bit(volumes, volume, case):
    kind, pose, whole, extra = CASES[case]
    ora, dev = volumes[volume + kind]
    hits = 0
    for size in IMAGES:
        K = tc.intrinsics(*size, whole_centre=whole or size == (1, 1))  # (the one pixel of 1 x 1 looks along the optical axis)
        stats = {}
        want = _restated(ora, K, pose, size, extra, stats)
        got = [x.cpu().numpy() for x in dev.raycast(K, pose, size, return_vertex=True, return_normal=True, return_color=True, **extra)]
        again = [x.cpu().numpy() for x in dev.raycast(K, pose, size, return_vertex=True, return_normal=True, return_color=True, **extra)]
        for name, w, g, a in zip(("depth", "vertex", "normal"), want, got, again):
            assert np.array_equal(_bits(g), _bits(w)), (case, size, name, int((_bits(g) != _bits(w)).sum()))
            assert np.array_equal(_bits(g), _bits(a)), (case, size, name, "two calls differ")
        assert np.array_equal(got[3], want[3]) and np.array_equal(got[3], again[3]), (case, size, "colour")
        depth_only = dev.raycast(K, pose, size, **extra)
        assert np.array_equal(_bits(depth_only.cpu().numpy()), _bits(want[0]))
        hits += int((want[0] > 0).sum())
        if size == (48, 64):  # the case is what its name says
            hit_share = float((want[0] > 0).mean())
            if case in ("corner", "coarse step"):
                assert hit_share > 0.4 and np.abs(want[2]).sum(axis=-1).astype(bool).mean() > 0.3 and want[3].any()
            elif case == "looking away":
                assert hit_share == 0.0
            elif case == "outside looking in":
                assert hit_share > 0.05
            elif case == "axis-parallel rays":
                assert hit_share > 0.05 and (want[0][:, 32] > 0).any() and (want[0][24, :] > 0).any()  # the column and the row with a zero component
            elif case == "one side, from behind the walls":
                assert stats["back"] > 0 and stats["invalid"] > 0 and hit_share < 0.5
            elif case == "z_near and z_far":
                full = _restated(ora, K, pose, size, {})[0]
                assert 0 < (want[0] > 0).sum() < (full > 0).sum()
                inside = want[0] > 0
                assert want[0][inside].min() >= 0.9 and want[0][inside].max() <= 1.15 + 1e-6
    if case == "looking away":
        assert hits == 0


def test_axis_parallel_rays_have_a_zero_component():
    """The premise of the case above: with no rotation and a whole-pixel principal point, the centre column's direction has x == 0 exactly."""
    K = tc.intrinsics(48, 64, whole_centre=True)
    assert (np.float32(32) - K[0, 2]) / K[0, 0] == 0 and (np.float32(24) - K[1, 2]) / K[1, 1] == 0
    assert np.array_equal(tc.axis_pose()[:3, :3], np.eye(3))


def test_untouched_volume_gives_zero_planes(gpu_ctx):
    from hive_amd import fusion
    vol = fusion.TSDFVolume(VOLUMES["cube32"], VOXEL, ctx=gpu_ctx)
    K = tc.intrinsics(24, 32)
    planes = vol.raycast(K, tc.corner_orbit(1)[0], (24, 32), return_vertex=True, return_normal=True, return_color=True)
    for p in planes:
        assert not p.cpu().numpy().any()


def test_slab_volume_is_refused(gpu_ctx):
    from hive_amd import _lib, fusion
    vol = fusion.TSDFVolume(VOLUMES["cube32"], VOXEL, ctx=gpu_ctx, x_range=(4, 20))
    with pytest.raises(_lib.HiveError) as err:
        vol.raycast(tc.intrinsics(24, 32), tc.corner_orbit(1)[0], (24, 32))
    assert err.value.code == _lib.ERR_INVALID


def test_bad_arguments_are_refused(gpu_ctx):
    from hive_amd import _lib, fusion
    vol = fusion.TSDFVolume(VOLUMES["cube32"], VOXEL, ctx=gpu_ctx)
    pose = tc.corner_orbit(1)[0]
    with pytest.raises(ValueError):
        vol.raycast(tc.intrinsics(24, 32), pose, (0, 32))
    for kw in ({"step": 0.0}, {"z_near": -1.0}):
        with pytest.raises(_lib.HiveError) as err:
            vol.raycast(tc.intrinsics(24, 32), pose, (24, 32), **kw)
        assert err.value.code == _lib.ERR_INVALID
