"""The fused TSDF sweep (hive_tsdf_integrate_batch on device frames: clip_row, build_worklist_multi_kernel, sort_worklist_kernel,
integrate_multi_kernel) against the C oracle, whole volumes bit for bit, at arbitrary camera poses, ragged shapes and special depths.
Every voxel the work list lets through runs the exact tests, so the sweep can only be wrong by leaving a voxel out or by addressing one
wrongly: comparing all three planes catches exactly that.  The scenes and their premises: tsdf_sweep_cases.py, checked without a GPU by
test_tsdf_sweep_cases_cpu.py."""
import numpy as np
import pytest

import tsdf_sweep_cases as cases

pytestmark = pytest.mark.gpu

WEIGHTS = (1.0, 0.37, 1.0)  # round mode 1: update forms <1, 2> (whole-number weights), <1, 0>, <1, 1>; round mode 0: <0, 1>, <0, 0>, <0, 1>


def _planes_equal(vol, planes, what=""):
    tsdf, color, weight = vol.get_volume(with_weight=True)
    assert np.array_equal(weight, planes[2]), f"weight volume differs {what}"
    assert np.array_equal(color, planes[1]), f"colour volume differs {what}"
    assert np.array_equal(tsdf, planes[0]), f"tsdf volume differs {what}"


def _device(scene, kind, frames=slice(None)):
    import torch
    return torch.from_numpy(scene["color"][frames]).cuda(), torch.from_numpy(scene["depth"][kind][frames]).cuda()


def _groups(scene, frames=slice(None)):
    return cases.predict_groups(scene["poses"][frames], cases.longest_side(scene["bounds"], scene["voxel"]))


@pytest.mark.parametrize("mode", ["0", "1", "2"])
@pytest.mark.parametrize("round_mode", [0, 1])
@pytest.mark.parametrize("cfg", cases.CONFIGS, ids=lambda c: c["name"])
def test_random_pose_groups_match_the_oracle(gpu_ctx, oracle_lib, monkeypatch, cfg, round_mode, mode):
    """Groups of every length around random poses (cameras inside, outside, behind and tilted against the volume; both row decompositions
    of the work-list kernel; fx != fy, principal point off centre), noise-like and patchy depth: three batches into one volume with
    observation weights 1, 0.37, 1 -- all five forms of integrate_multi_kernel between the two round modes -- under each mode of the per-row
    far cut; the groups as predicted and all three planes equal to the oracle's after every batch.  Beside it the single-frame kernel on
    the same frames, its update counts against the oracle's."""
    from hive_amd import fusion
    monkeypatch.setenv("HIVE_TSDF_ROW_FAR", mode)
    s = cases.random_pose_scene(cfg)
    groups = _groups(s)
    for kind in ("noise", "patchy"):
        ref = cases.oracle_run(oracle_lib, s, kind, round_mode, WEIGHTS)
        color_d, depth_d = _device(s, kind)
        vol = fusion.TSDFVolume(s["bounds"], s["voxel"], ctx=gpu_ctx, round_mode=round_mode)
        assert tuple(vol.vol_dim) == cfg["dims"]
        for k, w in enumerate(WEIGHTS):
            vol.integrate_batch(color_d, depth_d, s["K"], s["poses"], obs_weight=w)
            assert vol.last_batch_groups() == groups
            _planes_equal(vol, ref["passes"][k], f"({kind}, batch {k}, weight {w})")
        one = fusion.TSDFVolume(s["bounds"], s["voxel"], ctx=gpu_ctx, round_mode=round_mode)
        counts = [one.integrate(color_d[i], depth_d[i], s["K"], s["poses"][i], return_n_updated=True) for i in range(len(s["poses"]))]
        assert counts == ref["n_updated"], kind
        _planes_equal(one, ref["passes"][0], f"({kind}, single-frame kernel)")


@pytest.mark.parametrize("cfg", cases.CONFIGS + [cases.WIDE], ids=lambda c: c["name"])
def test_per_row_far_cut_only_shortens_the_work_list(gpu_ctx, oracle_lib, monkeypatch, cfg):
    """Patchy depth, one integrate_batch per predicted group so that every sweep's work list can be read back: forcing the per-row far cut
    on (HIVE_TSDF_ROW_FAR=2) gives no sweep a longer list than forcing it off (0) -- a cut can only shorten a row's interval -- and the
    oracle's volume either way.  In the wide configuration (five tile columns, near tiles on the left, the far pixel on the right) the list
    is strictly shorter for at least one sweep; the other images have 2 x 2 tiles, whose dilated table is the frame's maximum everywhere."""
    from hive_amd import fusion
    s = cases.random_pose_scene(cfg)
    groups = _groups(s)
    starts = cases.group_starts(groups)
    ref = cases.oracle_run(oracle_lib, s, "patchy", 1, WEIGHTS if cfg in cases.CONFIGS else (1.0,))
    color_d, depth_d = _device(s, "patchy")
    voxels = {}
    for mode in ("0", "2"):
        monkeypatch.setenv("HIVE_TSDF_ROW_FAR", mode)
        vol = fusion.TSDFVolume(s["bounds"], s["voxel"], ctx=gpu_ctx)
        voxels[mode] = []
        for st, g in zip(starts, groups):
            vol.integrate_batch(color_d[st:st + g], depth_d[st:st + g], s["K"], s["poses"][st:st + g])
            assert vol.last_batch_groups() == [g]
            voxels[mode].append(vol.last_sweep_voxels())
        _planes_equal(vol, ref["passes"][0], f"(mode {mode})")
    print("work-list voxels per sweep, cut off / on:", voxels["0"], voxels["2"])
    assert all(b <= a for a, b in zip(voxels["0"], voxels["2"]))
    assert sum(voxels["0"]) > 0
    if cfg is cases.WIDE:
        assert any(b < a for a, b in zip(voxels["0"], voxels["2"]))


@pytest.mark.parametrize("kind", ["noise", "patchy"])
def test_random_pose_groups_on_x_slabs(gpu_ctx, oracle_lib, kind):
    """The 70 x 61 x 80 grid cut at x = 0, 27, 28, 70 (rows per slab 27 * 61, 61, 42 * 61: the last quad of rows ragged in all three), the whole
    batch into each slab: the groups as predicted on every slab, and the slabs concatenated equal to the oracle's volume."""
    from hive_amd import fusion
    cfg = cases.CONFIGS[0]
    s = cases.random_pose_scene(cfg)
    groups = _groups(s)
    ref = cases.oracle_run(oracle_lib, s, kind, 1, WEIGHTS)["passes"][0]
    color_d, depth_d = _device(s, kind)
    cuts = [0, 27, 28, 70]
    parts = []
    for a, b in zip(cuts, cuts[1:]):
        slab = fusion.TSDFVolume(s["bounds"], s["voxel"], ctx=gpu_ctx, x_range=(a, b))
        assert tuple(slab.vol_dim) == (b - a, 61, 80)
        slab.integrate_batch(color_d, depth_d, s["K"], s["poses"])
        assert slab.last_batch_groups() == groups
        parts.append(slab.get_volume(with_weight=True))
    for k, plane in zip((0, 1, 2), ref):
        assert np.array_equal(np.concatenate([p[k] for p in parts], axis=0), plane)


def test_a_group_that_straddles_the_prepared_chunk(gpu_ctx, oracle_lib):
    """135 frames in one integrate_batch: frames are prepared 128 at a time, and the group of four at frame 127 does not fit the first
    chunk -- the batch prepares frames again from 127 on.  Groups [3] + [4] * 33 and the oracle's volume after 135 serial integrates."""
    from hive_amd import fusion
    s = cases.chunk_straddle_scene()
    ref = cases.oracle_run(oracle_lib, s, "noise")
    color_d, depth_d = _device(s, "noise")
    vol = fusion.TSDFVolume(s["bounds"], s["voxel"], ctx=gpu_ctx)
    assert tuple(vol.vol_dim) == (32, 32, 32)
    vol.integrate_batch(color_d, depth_d, s["K"], s["poses"])
    assert vol.last_batch_groups() == [3] + [4] * 33
    _planes_equal(vol, ref["passes"][0])


def test_frames_that_are_not_16_byte_aligned(gpu_ctx, oracle_lib):
    """The 48 x 64 frames (W % 4 == 0: the vector pre-pass when aligned) one float / one byte into larger device buffers: the batch takes the
    scalar pre-pass.  Same volume as the aligned run and as the oracle."""
    import torch
    from hive_amd import fusion
    cfg = cases.CONFIGS[1]
    s = cases.random_pose_scene(cfg)
    ref = cases.oracle_run(oracle_lib, s, "noise", 1, WEIGHTS)["passes"][0]
    color_d, depth_d = _device(s, "noise")
    n, H, W = depth_d.shape
    assert W % 4 == 0 and depth_d.data_ptr() % 16 == 0 and color_d.data_ptr() % 4 == 0
    depth_buf = torch.zeros(n * H * W + 4, dtype=torch.float32, device="cuda")
    color_buf = torch.zeros(n * H * W * 3 + 4, dtype=torch.uint8, device="cuda")
    depth_u, color_u = depth_buf[1:1 + n * H * W].view(n, H, W), color_buf[1:1 + n * H * W * 3].view(n, H, W, 3)
    depth_u.copy_(depth_d)
    color_u.copy_(color_d)
    assert depth_u.is_contiguous() and color_u.is_contiguous()
    assert depth_u.data_ptr() % 16 != 0 and color_u.data_ptr() % 4 != 0
    vols = []
    for c, d in ((color_d, depth_d), (color_u, depth_u)):
        vol = fusion.TSDFVolume(s["bounds"], s["voxel"], ctx=gpu_ctx)
        vol.integrate_batch(c, d, s["K"], s["poses"])
        assert vol.last_batch_groups() == _groups(s)
        _planes_equal(vol, ref)
        vols.append(vol.get_volume(with_weight=True))
    for a, b in zip(*vols):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("round_mode", [0, 1])
@pytest.mark.parametrize("kind", ["nan", "inf", "neg", "negzero", "all"])
def test_special_depth_values(gpu_ctx, oracle_lib, kind, round_mode):
    """NaN, +inf, -0.05 and -0.0 in a depth map do what the contract's tests make of them (the oracle): a NaN or +inf pixel updates every
    voxel in front of the camera that rounds to it -- far beyond the rest of the frame -- so it must count as +inf where the frame's tile
    maxima bound the work list.  Each value alone (beside +inf the frame's maximum is infinite already) and the four together; the
    single-frame kernel with its update counts, a fused pair and a fused four."""
    from hive_amd import fusion
    s = cases.special_depth_scene(kind)
    color_d, depth_d = _device(s, "plane")
    ref = cases.oracle_run(oracle_lib, s, "plane", round_mode)
    one = fusion.TSDFVolume(s["bounds"], s["voxel"], ctx=gpu_ctx, round_mode=round_mode)
    counts = [one.integrate(s["color"][i], s["depth"]["plane"][i], s["K"], s["poses"][i], return_n_updated=True) for i in range(4)]
    print("updates per frame:", counts, "oracle:", ref["n_updated"])
    assert counts == ref["n_updated"]
    _planes_equal(one, ref["passes"][0], "(single-frame kernel)")
    for nf in (2, 4):
        ref_n = cases.oracle_run(oracle_lib, s, "plane", round_mode, frames=range(nf))
        vol = fusion.TSDFVolume(s["bounds"], s["voxel"], ctx=gpu_ctx, round_mode=round_mode)
        vol.integrate_batch(color_d[:nf], depth_d[:nf], s["K"], s["poses"][:nf])
        assert vol.last_batch_groups() == [nf]
        _planes_equal(vol, ref_n["passes"][0], f"(fused {nf})")


@pytest.mark.parametrize("round_mode", [0, 1])
def test_volume_far_from_the_origin(gpu_ctx, oracle_lib, round_mode):
    """World coordinates around z = 131072 m (float32 steps of a quarter voxel): the row clip's conversion of a cut position into a voxel
    index is off by more than its half-pixel padding covers, and only the widening of the interval by 2 / 3 voxels keeps the updated voxels
    on the work list (test_tsdf_sweep_cases_cpu.py counts them).  Three fused groups of four and the single-frame kernel's update counts."""
    from hive_amd import fusion
    s = cases.far_offset_scene()
    ref = cases.oracle_run(oracle_lib, s, "noise", round_mode)
    color_d, depth_d = _device(s, "noise")
    vol = fusion.TSDFVolume(s["bounds"], s["voxel"], ctx=gpu_ctx, round_mode=round_mode)
    assert tuple(vol.vol_dim) == (40, 36, 48)
    vol.integrate_batch(color_d, depth_d, s["K"], s["poses"])
    assert vol.last_batch_groups() == [4, 4, 4]
    _planes_equal(vol, ref["passes"][0], "(fused)")
    one = fusion.TSDFVolume(s["bounds"], s["voxel"], ctx=gpu_ctx, round_mode=round_mode)
    counts = [one.integrate(color_d[i], depth_d[i], s["K"], s["poses"][i], return_n_updated=True) for i in range(len(s["poses"]))]
    print("updates per frame:", counts, "oracle:", ref["n_updated"])
    assert counts == ref["n_updated"]
    _planes_equal(one, ref["passes"][0], "(single-frame kernel)")


@pytest.mark.parametrize("round_mode", [0, 1])
def test_degenerate_volume(gpu_ctx, oracle_lib, round_mode):
    """5 x 3 x 3 voxels: 15 rows (the fourth quad of rows has three), every row a single quad of three voxels whose fourth lies in the
    next row -- or, for the last row, past the end of the planes.  Fused groups of two, three and four against the oracle."""
    from hive_amd import fusion
    s = cases.degenerate_scene()
    color_d, depth_d = _device(s, "noise")
    for nf in (2, 3, 4):
        ref = cases.oracle_run(oracle_lib, s, "noise", round_mode, frames=range(nf))
        vol = fusion.TSDFVolume(s["bounds"], s["voxel"], ctx=gpu_ctx, round_mode=round_mode)
        assert tuple(vol.vol_dim) == (5, 3, 3)
        vol.integrate_batch(color_d[:nf], depth_d[:nf], s["K"], s["poses"][:nf])
        assert vol.last_batch_groups() == [nf]
        _planes_equal(vol, ref["passes"][0], f"(fused {nf})")
