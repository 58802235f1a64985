"""DPT on the MI355X at the size the benchmark runs (480 x 640, 1,201 tokens, batches of frames): the HIP engine
(MFMA ViT blocks and convolutions, fused channels-last glue, fused depth head; in bfloat16 AND in float16, the type the reference
runs: ``model.half()``, /root/reference/hive/dataset_adaptors.py:1394-1401) against

  * the float32 PyTorch formulation of the same module, stage by stage, with seeded weights that give every stage a
    usable dynamic range (tests/dpt_weights.py) -- relative Frobenius error per stage and depth error in millimetres,
    the unit the reference hands off (/root/reference/hive/dataset_adaptors.py:1432-1433);
  * golden activations of an independent implementation of the published architecture (tests/golden/dpt_*_hf.npz);
  * the driver `estimate_depth_dpt` end to end (checkpoint on disk -> 16-bit PNGs), native and non-native frame sizes.

Stated tolerances (bf16 network, float32 tail; measured values in DESIGN.md section 3):  relative Frobenius error <= 5 % for
the tokens behind the 16 bottleneck blocks of the ResNetV2 stem, <= 2.5 % behind the 12 transformer blocks and in the decoder,
and never more than 1.2 x what PyTorch's own bf16 operators lose on the same weights; depth error: median <= 20 mm, 99th
percentile <= 120 mm over a 1.2 .. 7.3 m range (bf16 keeps 8 significant bits: one ulp of a feature is 0.4 % of its value).
float16 network (11 significant bits): every one of these bounds divided by EIGHT (HALF_TIGHT below).

The HIP engine is bit-reproducible run to run (no atomics, fixed accumulation orders; tools/diag_determinism.py: 0.0 mm between
identical forwards) -- PyTorch's own bf16 operators are not (MIOpen's convolutions: ~250 mm between two runs on these weights),
which is why comparisons against the PyTorch-op engine use tolerances.
"""
import os

import numpy as np
import pytest
import torch

from dpt_weights import seeded_init, seeded_input, state_checksum

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SCALE, SHIFT = 0.000305, 0.1378
HALF_TIGHT = {torch.bfloat16: 1.0, torch.float16: 0.125}  # float16 carries 3 more significant bits than bfloat16


@pytest.fixture(params=["bfloat16", "float16"])
def half(request):
    """The 16-bit type of the network under test."""
    return getattr(torch, request.param)


def _rel(a, b):
    a, b = torch.as_tensor(a).float().cpu(), torch.as_tensor(b).float().cpu()
    return float((a - b).norm() / b.norm())


def _pair(backbone="vitb_rn50_384", seed=1234, scale=SCALE, shift=SHIFT, invert=True, dtype=torch.bfloat16):
    """(float32 PyTorch-formulation model, 16-bit channels-last HIP-engine model) with the same seeded weights."""
    from hive_amd.dpt.models import DPTDepthModel
    ref = DPTDepthModel(path=None, scale=scale, shift=shift, invert=invert, engine="torch", backbone=backbone).eval()
    seeded_init(ref, seed=seed)
    hip = DPTDepthModel(path=None, scale=scale, shift=shift, invert=invert, engine="hip", backbone=backbone).eval()
    hip.load_state_dict(ref.state_dict())
    hip = hip.to(memory_format=torch.channels_last).to(dtype).cuda()
    return ref.cuda(), hip


def _net_input(x, dtype=torch.bfloat16):
    return x.cuda().to(dtype).contiguous(memory_format=torch.channels_last)


def test_per_stage_480x640_batch4(gpu_ctx, half):
    from hive_amd.dpt.models import DPTDepthModel
    tight = HALF_TIGHT[half]
    ref, hip = _pair(dtype=half)
    # the same network in the same 16-bit type with PyTorch's own operators (MIOpen / rocBLAS): what that type costs on these weights,
    # whoever computes it
    tor = DPTDepthModel(path=None, scale=SCALE, shift=SHIFT, invert=True, engine="torch").eval()
    tor.load_state_dict(ref.state_dict())
    tor = tor.to(memory_format=torch.channels_last).to(half).cuda()
    x = seeded_input(4, 480, 640, seed=7).bfloat16().float()  # all models see the same input (bfloat16 values: exact in float16 too)
    s_ref, s_hip, s_tor = {}, {}, {}
    with torch.no_grad():
        d_ref = ref(x.cuda(), stages=s_ref)
        d_hip = hip(_net_input(x, half), stages=s_hip)
        tor(_net_input(x, half), stages=s_tor)
    assert s_hip["tokens"].shape == (4, 30 * 40 + 1, 768), "480 x 640 -> 30 x 40 token grid + class token"
    bounds = {"tokens": 5e-2, "tap_3": 2.5e-2, "tap_4": 2.5e-2, "layer_1": 1.5e-2, "layer_2": 2.5e-2, "layer_3": 2.5e-2, "layer_4": 2.5e-2,
              "path_4": 2.5e-2, "path_3": 2.5e-2, "path_2": 2.5e-2, "path_1": 2.5e-2, "head_in": 2.5e-2}
    report = {}
    for name, bound in bounds.items():
        assert s_hip[name].shape == s_ref[name].shape, name
        assert s_hip[name].dtype == half, name
        assert torch.isfinite(s_hip[name].float()).all(), name
        report[name] = _rel(s_hip[name], s_ref[name])
    err_mm = ((d_hip - d_ref).abs() * 1000.0).flatten().cpu()
    report["depth_mm_median"] = float(err_mm.median())
    report["depth_mm_p99"] = float(torch.quantile(err_mm[::7], 0.99))
    report["depth_range_m"] = (float(d_ref.min()), float(d_ref.max()))
    print(f"per-stage relative Frobenius error, HIP {half} vs float32:", {k: (round(v, 6) if isinstance(v, float) else v) for k, v in report.items()})
    for name, bound in bounds.items():
        assert report[name] <= tight * bound, f"{name}: relative error {report[name]:.4g} > {tight * bound}"
        # the hand-written kernels must not be less accurate than PyTorch's own operators in the same type on the same weights
        err_torch = _rel(s_tor[name], s_ref[name])
        assert report[name] <= 1.2 * err_torch + tight * 2e-3, f"{name}: HIP {report[name]:.4g} vs PyTorch-{half} {err_torch:.4g}"
    assert d_hip.shape == (4, 480, 640) and d_hip.dtype == torch.float32
    assert float(d_ref.max()) - float(d_ref.min()) > 4.0, "seeded head must span metres, not sit on the clamp"
    assert float((d_ref > 7.25).float().mean()) < 0.02
    assert report["depth_mm_median"] <= tight * 20.0 and report["depth_mm_p99"] <= tight * 120.0, report


def test_per_stage_480x640_batch1(gpu_ctx, half):
    """The reference's LITERAL call pattern -- one frame per forward at 480 x 640 (/root/reference/hive/dataset_adaptors.py:1406-1419) -- takes a code path of its
    own: launches that do not fill the chip run on the four-stage-ring kernels and split their long K loops (csrc/mfma_pipe.hpp).  Same per-stage bounds
    against the float32 network as the batch of four above, and the launch counters say that path really ran."""
    tight = HALF_TIGHT[half]
    ref, hip = _pair(dtype=half)
    x = seeded_input(4, 480, 640, seed=7).bfloat16().float()[2:3].contiguous()  # one frame of the batch-of-four test's input
    s_ref, s_hip = {}, {}
    ctx = gpu_ctx
    with torch.no_grad():
        d_ref = ref(x.cuda(), stages=s_ref)
        hip(_net_input(x, half))  # (first call: weight packing, workspaces)
        ctx.launch_stats(reset=True)
        d_hip = hip(_net_input(x, half), stages=s_hip)
    n_split, n_deep = ctx.launch_stats()
    assert n_split >= 12 and n_deep >= 60, f"one frame must take the split-K ({n_split} launches) and deep-ring ({n_deep}) paths"
    bounds = {"tokens": 5e-2, "tap_3": 2.5e-2, "tap_4": 2.5e-2, "layer_1": 1.5e-2, "layer_2": 2.5e-2, "layer_3": 2.5e-2, "layer_4": 2.5e-2,
              "path_4": 2.5e-2, "path_3": 2.5e-2, "path_2": 2.5e-2, "path_1": 2.5e-2, "head_in": 2.5e-2}
    report = {name: _rel(s_hip[name], s_ref[name]) for name in bounds}
    err_mm = ((d_hip - d_ref).abs() * 1000.0).flatten().cpu()
    report["depth_mm_median"], report["depth_mm_p99"] = float(err_mm.median()), float(torch.quantile(err_mm[::7], 0.99))
    print(f"per-stage relative Frobenius error at ONE frame, HIP {half} vs float32:", {k: round(v, 6) for k, v in report.items()}, "split-K launches", n_split, "deep-ring", n_deep)
    for name, bound in bounds.items():
        assert s_hip[name].dtype == half and torch.isfinite(s_hip[name].float()).all(), name
        assert report[name] <= tight * bound, f"{name}: relative error {report[name]:.4g} > {tight * bound}"
    assert report["depth_mm_median"] <= tight * 20.0 and report["depth_mm_p99"] <= tight * 120.0, report
    # deterministic mode: neither path whose use depends on the batch size -- no split-K launch
    ctx.set_deterministic(True)
    try:
        ctx.launch_stats(reset=True)
        with torch.no_grad():
            d_det = hip(_net_input(x, half))
        assert ctx.launch_stats()[0] == 0
        assert _median_mm(d_det, d_hip) <= tight * 20.0
    finally:
        ctx.set_deterministic(False)


def test_reference_call_sequence_runs_on_the_hip_engine(gpu_ctx):
    """The reference's literal sequence (dataset_adaptors.py:1366-1401, 1415-1419): construct, eval, channels_last, `.half()`, to the
    device, a float16 sample -> depth.  It runs on the hand-written float16 kernels; a float32 model (the reference's
    optimize=False) RAISES on the HIP engine instead of being down-cast or handed to PyTorch operators; and the network object
    (hive_dpt_forward) launches nothing but this library's kernels (kernel names from torch's profiler)."""
    from hive_amd import _lib, depth as depth_mod
    from hive_amd.dpt.models import DPTDepthModel
    model = DPTDepthModel(path=None, scale=SCALE, shift=SHIFT, invert=True, backbone="vitb_rn50_384", non_negative=True, enable_attention_hooks=False)
    seeded_init(model, seed=3)
    ref32 = DPTDepthModel(path=None, scale=SCALE, shift=SHIFT, invert=True, engine="torch").eval()
    ref32.load_state_dict(model.state_dict())
    model.eval()
    model = model.to(memory_format=torch.channels_last)
    model = model.half()
    model.to("cuda")
    x = seeded_input(2, 96, 128, seed=9)
    sample = x.to("cuda").to(memory_format=torch.channels_last).half()
    with torch.no_grad():
        prediction = model.forward(sample)
        d32 = ref32.cuda()(x.cuda())
    assert prediction.shape == (2, 96, 128) and torch.isfinite(prediction).all()
    assert _median_mm(prediction, d32) <= 4.0, "float16 on the HIP engine vs the float32 network"
    with pytest.raises(_lib.HiveError, match="not covered by the HIP kernels"):
        model.float()(x.cuda().contiguous(memory_format=torch.channels_last))  # optimize=False: float32 needs engine="torch", stated loudly
    model = model.half()
    with pytest.raises(_lib.HiveError):
        model(sample.contiguous())  # not channels-last
    frames = torch.randint(0, 256, (2, 96, 128, 3), dtype=torch.uint8, device="cuda")
    model.forward_frames(frames, max_depth=10.0)  # builds the network object, sizes its arena
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            with torch.no_grad():
                model.forward_frames(frames, max_depth=10.0)
            torch.cuda.synchronize()
        names = [e.key for e in prof.key_averages() if getattr(e, "device_type", None) is not None and "cuda" in str(e.device_type).lower()]
    except Exception as exc:  # the profiler is not what is under test
        pytest.skip(f"torch.profiler unavailable on this box: {exc}")
    kernels = [n for n in names if not n.lower().startswith(("memcpy", "memset", "hipmemcpy", "hipmemset"))]
    if not kernels:
        pytest.skip("torch.profiler recorded no device kernels on this box")
    foreign = [n for n in kernels if any(t in n for t in ("at::native", "at::cuda", "Cijk_", "ck::", "igemm", "miopen", "MIOpen", "rocblas", "elementwise_kernel"))]
    assert not foreign, f"hive_dpt_forward launched kernels that are not this library's: {foreign[:5]}"
    assert any("gemm" in n or "conv_kernel" in n for n in kernels), kernels[:10]


def _median_mm(a, b):
    return float(((a - b).abs() * 1000.0).flatten().median())


def test_batch_independence_and_determinism(gpu_ctx, monkeypatch):
    """Frame i of a batch of 6 == the same frame run alone (no cross-frame leakage through the padded token rows, the
    batched GroupNorm statistics or the attention masks); the hand-written ViT engine is bit-reproducible.  A lone frame's fc2 GEMMs split
    their K loop over several workgroups (csrc/mfma_pipe.hpp splitk_combine) and its attention launches their keys over two groups of waves (vit.hip
    attention_kernel KS = 2) -- other, fixed, orders of float32 additions -- so the bitwise comparison runs with HIVE_SPLITK=0 HIVE_ATT_KSPLIT=0; with the
    splits the frame alone is reproducible and within rounding noise of the frame in the batch."""
    from hive_amd.dpt.vit_engine import VitEngine
    _, hip = _pair()
    eng = VitEngine(hip.pretrained.model, ctx=gpu_ctx)
    torch.manual_seed(7)
    tokens = torch.randn(6, 1201, 768, device="cuda").bfloat16()
    t_all = eng.forward(tokens, taps=(8, 11))
    t_again = eng.forward(tokens, taps=(8, 11))
    t_split = eng.forward(tokens[4:5].contiguous(), taps=(8, 11))
    t_split_again = eng.forward(tokens[4:5].contiguous(), taps=(8, 11))
    monkeypatch.setenv("HIVE_SPLITK", "0")
    monkeypatch.setenv("HIVE_ATT_KSPLIT", "0")
    t_one = eng.forward(tokens[4:5].contiguous(), taps=(8, 11))
    monkeypatch.delenv("HIVE_SPLITK")
    monkeypatch.delenv("HIVE_ATT_KSPLIT")
    assert torch.equal(t_all[0], t_again[0]) and torch.equal(t_all[1], t_again[1]), "ViT engine: two runs differ"
    assert torch.equal(t_all[1][4:5], t_one[1]), "ViT engine: an image in a batch differs from the image alone"
    assert torch.equal(t_split[0], t_split_again[0]) and torch.equal(t_split[1], t_split_again[1]), "ViT engine (split K): two runs differ"
    # Two orders of float32 additions in 12 of the 48 GEMMs, with bfloat16 roundings of the activations in between: a sum that moves by one float32 ulp flips
    # the 16-bit rounding of ~1 in 2^16 outputs, and twelve blocks of residual stream carry the flips forward.  Measured once over 8 token seeds
    # (tools/diag_splitk_bound.py -> profiles/r05_diag_splitk_bound.log): 0.0066 every time in bfloat16 (0.00084 in float16: 8 x finer) -- a property of
    # the weights' gain through the blocks, not of the tokens.  The bound is that value + 50 %.
    assert _rel(t_split[1].float(), t_one[1].float().cpu().numpy()) < 1e-2
    x = _net_input(seeded_input(6, 480, 640, seed=11))
    with torch.no_grad():
        d_all = hip(x)
        d_again = hip(x)
        d_one = hip(x[4:5].contiguous(memory_format=torch.channels_last))
    # whole model: every kernel of the HIP engine has a fixed accumulation order -> two runs are bit-identical
    assert torch.equal(d_all, d_again), "the HIP engine must be reproducible run to run"
    # a frame in a batch vs the frame alone: same per-pixel arithmetic, but the lone frame splits its long K loops and the GroupNorm partial-sum slabs are cut
    # from the start of the batch: bf16 rounding noise.  Measured over 8 inputs (same log): median 5.4-8.7 mm in bfloat16 (0.7-0.9 mm in float16), against
    # 9.4 mm of either form vs the float32 network.  Bound: the largest + 40 %.
    assert _median_mm(d_all[4], d_one[0]) <= 12.0


@pytest.mark.parametrize("fixture", ["dpt_hybrid_hf.npz", "dpt_large_hf.npz"])
def test_hip_engine_against_independent_implementation(gpu_ctx, fixture):
    gold = np.load(os.path.join(GOLDEN, fixture))
    ref, hip = _pair(backbone=str(gold["backbone"]), seed=int(gold["seed"]), scale=1.0, shift=0.0, invert=False)
    assert state_checksum(ref) == str(gold["state_sha256"]), "seeded weights differ from the fixture's: rerun tests/golden/make_dpt_golden.py"
    x = torch.from_numpy(gold["x"].astype(np.float32))
    stages = {}
    with torch.no_grad():
        inv = hip(_net_input(x), stages=stages)
        inv_ref = ref(x.cuda())
    assert _rel(inv_ref, gold["inv_depth"]) < 1e-3, "float32 formulation on the GPU vs the fixture"
    assert _rel(stages["tap_4"], gold["tap_4"].astype(np.float32)) < 2.5e-2
    assert _rel(stages["path_4"], gold["path_4"].astype(np.float32)) < 3e-2
    assert _rel(stages["path_1"].float().mean(dim=1), gold["path_1_mean"]) < 3e-2
    assert _rel(inv, gold["inv_depth"]) < 3e-2


def test_hip_engine_against_independent_implementation_at_the_benchmark_size(gpu_ctx, half):
    """480 x 640 (1,201 tokens), both element types, against the golden activations of the INDEPENDENT implementation
    (tests/golden/dpt_hybrid_hf_480x640.npz: HuggingFace's DPT with the same seeded weights; sub-sampled views) -- not against this
    build's own float32 formulation.  Bounds: the per-stage ones of `test_per_stage_480x640_batch4` (float16: divided by eight)."""
    import hashlib
    gold = np.load(os.path.join(GOLDEN, "dpt_hybrid_hf_480x640.npz"))
    b, h, w = (int(v) for v in gold["shape"])
    x = seeded_input(b, h, w, seed=int(gold["x_seed"])).half().float()
    assert hashlib.sha256(x.numpy().astype(np.float16).tobytes()).hexdigest() == str(gold["x_sha256"])
    ref, hip = _pair(backbone=str(gold["backbone"]), seed=int(gold["seed"]), scale=1.0, shift=0.0, invert=False, dtype=half)
    assert state_checksum(ref) == str(gold["state_sha256"])
    tight = HALF_TIGHT[half]
    stages = {}
    with torch.no_grad():
        inv = hip(_net_input(x, half), stages=stages)
    rep = {"tap_3_mean": _rel(stages["tap_3"].float().mean(dim=2), gold["tap_3_mean"]), "tap_4": _rel(stages["tap_4"][:, ::16], gold["tap_4_s16"].astype(np.float32)),
           "path_4": _rel(stages["path_4"], gold["path_4"].astype(np.float32)), "path_1_mean": _rel(stages["path_1"].float().mean(dim=1)[:, ::2, ::2], gold["path_1_mean_s2"]),
           "head_in_mean": _rel(stages["head_in"].float().mean(dim=1)[:, ::2, ::2], gold["head_in_mean_s2"]), "inv_depth": _rel(inv[:, ::4, ::4], gold["inv_depth_s4"])}
    print(f"HIP {half} vs the independent implementation at 480 x 640:", {k: round(v, 6) for k, v in rep.items()})
    assert rep["tap_4"] <= tight * 2.5e-2 and rep["path_4"] <= tight * 2.5e-2 and rep["inv_depth"] <= tight * 3e-2, rep
    assert max(rep["path_1_mean"], rep["head_in_mean"]) <= tight * 3e-2, rep
    # (the channel mean of the tokens nearly cancels -- |mean| is a few per cent of the tokens' scale -- so its RELATIVE error is the
    # least well conditioned figure here: measured 0.055 / 0.0055)
    assert rep["tap_3_mean"] <= tight * 8e-2, rep


def test_dpt_large_1080p_network_size(gpu_ctx):
    """BASELINE config 4's network: DPT-Large on a 1920 x 1080 frame = 480 x 864 network input by the reference's resize
    rule (30 x 54 + 1 = 1,621 tokens, d = 1024, 16 heads, 24 blocks through the same HIP engine)."""
    from hive_amd.dpt import transforms as T
    ref, hip = _pair(backbone="vitl16_384")
    r = T.Resize(640, 480, resize_target=None, keep_aspect_ratio=True, ensure_multiple_of=32, resize_method="minimal")
    w, h = r.get_size(1920, 1080)
    assert (w, h) == (864, 480)
    x = seeded_input(1, h, w, seed=3).bfloat16().float()
    s_ref, s_hip = {}, {}
    with torch.no_grad():
        d_ref = ref(x.cuda(), stages=s_ref)
        d_hip = hip(_net_input(x), stages=s_hip)
    assert s_hip["tokens"].shape == (1, 30 * 54 + 1, 1024)
    rep = {k: _rel(s_hip[k], s_ref[k]) for k in ("tap_3", "tap_4", "layer_1", "layer_4", "path_1", "head_in")}
    err_mm = ((d_hip - d_ref).abs() * 1000.0).flatten().cpu()
    print("DPT-Large 480 x 864:", {k: round(v, 5) for k, v in rep.items()}, "depth mm median", float(err_mm.median()))
    assert max(rep.values()) <= 3.5e-2, rep
    assert float(err_mm.median()) <= 20.0


def test_estimate_depth_dpt_end_to_end(gpu_ctx, tmp_path, monkeypatch):
    """The driver the reference calls (dataset_adaptors.py:225): checkpoint from $WEIGHTS_PATH, every frame of the dataset ->
    `%06d.png` (uint16 millimetres, truncated).  640 x 480 frames take the on-device preprocessing; another size goes through
    Resize + the nearest-neighbour resize back (:1421-1426)."""
    from PIL import Image
    from hive_amd import depth as depth_mod
    from hive_amd.dpt.models import DPTDepthModel
    src = DPTDepthModel(path=None, engine="torch").eval()
    seeded_init(src, seed=21)
    wdir = tmp_path / "weights"
    wdir.mkdir()
    torch.save(src.state_dict(), str(wdir / "dpt_hybrid_nyu.pt"))
    monkeypatch.setenv("WEIGHTS_PATH", str(wdir))
    rng = np.random.default_rng(0)

    def frames(n, h, w):
        base = (seeded_input(n, h, w, seed=h).permute(0, 2, 3, 1).numpy() * 0.5 + 0.5) * 255.0
        return [np.clip(base[i] + rng.normal(0, 2, base[i].shape), 0, 255).astype(np.uint8) for i in range(n)]

    model = depth_mod.build_model(str(wdir / "dpt_hybrid_nyu.pt"), dtype=None, engine="torch")  # the float32 network (PyTorch operators): the yardstick
    assert model.load_report == ([], []), "load() must consume every key of the checkpoint"
    for (h, w), n in (((480, 640), 5), ((200, 320), 3)):
        data = frames(n, h, w)
        out = tmp_path / f"depth_{h}"
        depth_mod.estimate_depth_dpt(data, str(out), batch_size=4)  # optimize=True: float16 on the HIP engine; 5 frames, batch 4: a ragged last batch
        assert sorted(os.listdir(out)) == [f"{i:06d}.png" for i in range(n)]
        for i in (0, n - 1):
            png = np.asarray(Image.open(out / f"{i:06d}.png"))
            assert png.dtype == np.uint16 and png.shape == (h, w)
            # the same frame through the float32 network with the reference's pre- and post-processing (:1407-1426)
            with torch.no_grad():
                arr = depth_mod.make_transform()({"image": data[i] / 255.0})["image"]
                assert arr.shape == ((3, 480, 640) if (h, w) == (480, 640) else (3, 384, 640))
                pred = model(torch.from_numpy(arr[None]).cuda())
                if pred.shape[-2:] != (h, w):
                    pred = torch.nn.functional.interpolate(pred.unsqueeze(1), size=(h, w), mode="nearest").squeeze(1)
            expect = (pred[0] * 1000.0).cpu().numpy().astype(np.uint16)  # the reference's truncation (:1432-1433)
            diff = np.abs(png.astype(np.int32) - expect.astype(np.int32))
            # float16 network vs float32 network on the same weights and frame: millimetres
            assert np.median(diff) <= 4 and np.percentile(diff, 99) <= 25, (np.median(diff), np.percentile(diff, 99))
            assert 400 < png.min() and png.max() <= 7257, "depth = 1 / (scale x + shift) <= 7.257 m (SURVEY.md §8 a-1)"
    # the bfloat16 kernels through the same driver; optimize=False = the float32 network on PyTorch operators, as the reference's
    data = frames(2, 480, 640)
    for kwargs, limit in ((dict(dtype=torch.bfloat16), 25), (dict(optimize=False), 1)):
        out = tmp_path / f"depth_{limit}"
        depth_mod.estimate_depth_dpt(data, str(out), batch_size=2, **kwargs)
        png = np.asarray(Image.open(out / "000001.png"))
        with torch.no_grad():
            arr = depth_mod.make_transform()({"image": data[1] / 255.0})["image"]
            expect = (model(torch.from_numpy(arr[None]).cuda())[0] * 1000.0).cpu().numpy().astype(np.uint16)
        assert np.median(np.abs(png.astype(np.int32) - expect.astype(np.int32))) <= limit, kwargs


def test_forward_on_a_side_stream_matches_default_stream(gpu_ctx):
    """`with torch.cuda.stream(s)`: the hive kernels must queue on the stream the surrounding torch ops use (the context
    re-binds to torch's current stream).  Unordered streams would let the ViT engine read tokens MIOpen is still writing."""
    from hive_amd.dpt.vit_engine import VitEngine
    _, hip = _pair()
    x = _net_input(seeded_input(2, 96, 128, seed=5))
    tokens = torch.randn(2, 301, 768, device="cuda").bfloat16()
    with torch.no_grad():
        d0 = hip(x)
        eng = VitEngine(hip.pretrained.model)  # default context of this thread: follows torch's current stream
        t0 = eng.forward(tokens, taps=(11,))[0]
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            filler = torch.randn(4096, 4096, device="cuda") @ torch.randn(4096, 4096, device="cuda")  # keeps the side stream busy
            tok_side = tokens * 1.0  # produced ON the side stream, behind the GEMM
            t1 = eng.forward(tok_side, taps=(11,))[0]
            d1 = hip(x)
        side.synchronize()
        d2 = hip(x)  # and back on the default stream
        t2 = eng.forward(tokens, taps=(11,))[0]
    assert torch.equal(t0, t1) and torch.equal(t0, t2), "ViT engine ran on another stream than its input's producer"
    assert _median_mm(d0, d1) <= 20.0 and _median_mm(d0, d2) <= 20.0 and torch.isfinite(filler).all()


def test_engine_follows_weight_updates(gpu_ctx):
    """The ViT engine packs private copies of biases / LayerNorm parameters: loading other weights must invalidate it."""
    from hive_amd.dpt.models import DPTDepthModel
    _, hip = _pair(seed=1)
    x = _net_input(seeded_input(1, 96, 128, seed=5))
    with torch.no_grad():
        d_a = hip(x)
        other = DPTDepthModel(path=None, scale=SCALE, shift=SHIFT, invert=True, engine="torch").eval()
        seeded_init(other, seed=2)
        hip.load_state_dict(other.state_dict())
        d_b = hip(x)
        fresh = DPTDepthModel(path=None, scale=SCALE, shift=SHIFT, invert=True, engine="hip").eval()
        fresh.load_state_dict(other.state_dict())
        fresh = fresh.to(memory_format=torch.channels_last).to(torch.bfloat16).cuda()
        d_c = fresh(x)
    assert _median_mm(d_a, d_b) > 100.0, "the two seeds must give different depth maps"
    assert _median_mm(d_b, d_c) <= 20.0, "stale packed parameters in the ViT engine after load_state_dict"


def test_weights_updated_in_place_through_the_c_abi(gpu_ctx):
    """hive_vit_create / hive_dpt_create SNAPSHOT what the folded LayerNorm needs (gamma o W of qkv / fc1, the constant rows); proj / fc2 are read live
    (include/hive_mi355x.h, "weight snapshot contract").  A C-ABI caller that overwrites the table's tensors in place must call
    hive_dpt_weights_modified: without it the next forward mixes old and new weights, with it the object equals one built from the new weights."""
    from hive_amd.dpt.native import NativeDPT
    _, hip = _pair(dtype=torch.float16, seed=21)
    frames = torch.randint(0, 256, (2, 96, 128, 3), dtype=torch.uint8, device="cuda")
    native = NativeDPT(hip, ctx=gpu_ctx)
    with torch.no_grad():
        before = native.forward(frames)[0].clone()
        # overwrite block 3's norm1 gain, qkv and proj weights IN PLACE, directly in the tensors whose addresses the table holds
        idx = {n.decode(): i for i, n in enumerate(native._names)}
        for name, factor in (("pretrained.model.blocks.3.norm1.weight", 1.5), ("pretrained.model.blocks.3.attn.qkv.weight", 0.5),
                             ("pretrained.model.blocks.3.attn.proj.weight", 2.0), ("pretrained.model.blocks.7.mlp.fc1.bias", 3.0)):
            native._keep[idx[name]].mul_(factor)
        stale = native.forward(frames)[0].clone()
        native.weights_modified()
        fresh = native.forward(frames)[0].clone()
        rebuilt = NativeDPT(hip, ctx=gpu_ctx)  # (the model's parameters share storage with the table's tensors or were re-packed from them)
        for name in ("pretrained.model.blocks.3.norm1.weight", "pretrained.model.blocks.7.mlp.fc1.bias"):  # float32 copies in the table: carry them over
            rebuilt._keep[{n.decode(): i for i, n in enumerate(rebuilt._names)}[name]].copy_(native._keep[idx[name]])
        rebuilt.weights_modified()
        want = rebuilt.forward(frames)[0]
    assert not torch.equal(before, fresh), "the overwritten weights must change the depth"
    assert torch.equal(fresh, want), "after hive_dpt_weights_modified the object must equal one built from the new weights"
    assert not torch.equal(stale, fresh), "without the call the folded copies are stale (that is the contract the header states)"
    native.close()
    rebuilt.close()


def test_native_network_object_equals_python_orchestration(gpu_ctx, half):
    """hive_dpt_create / forward / destroy (the whole DPT-Hybrid + pre-processing + depth hand-off behind ONE C-ABI call,
    csrc/dpt_net.hip) against the same kernels orchestrated from Python layer by layer: bit-identical depth, millimetres and
    metres (both paths are reproducible), at the benchmark's frame size and at a second size; rebuilt after a weight update."""
    from hive_amd import depth as depth_mod
    _, hip = _pair(dtype=half)
    rng = np.random.default_rng(1)
    for (b, h, w) in ((3, 480, 640), (2, 96, 160)):
        frames = torch.from_numpy(rng.integers(0, 256, (b, h, w, 3), dtype=np.uint8)).cuda()
        with torch.no_grad():
            d_py, mm_py, m_py = hip(depth_mod.preprocess_on_device(frames, half), handoff=(10.0,))
            d_c, mm_c, m_c = hip.forward_frames(frames, max_depth=10.0)
        assert d_c.shape == (b, h, w) and torch.isfinite(d_c).all()
        assert torch.equal(d_c, d_py), f"depth differs by up to {float((d_c - d_py).abs().max()) * 1000:.3f} mm"
        assert torch.equal(mm_c, mm_py) and torch.equal(m_c, m_py)
    nat = hip.native()
    assert hip.native() is nat, "the native object is cached while the parameters are unchanged"
    # the activation arena releases a map behind its last consumer: 3 frames of 480 x 640 need well under the 1.2 GB their maps total
    assert 0 < nat.arena_bytes() < 450e6, nat.arena_bytes()
    with torch.no_grad():
        hip.scratch.output_conv[4].bias.add_(50.0)
        d2, _, _ = hip.forward_frames(frames, max_depth=10.0)
    assert hip.native() is not nat and not torch.equal(d2, d_c), "a parameter update must rebuild the native network"
    with pytest.raises(Exception):
        hip.forward_frames(frames[:, :90], max_depth=10.0)  # 90 rows: not a multiple of 32


def test_large_batch_paths_of_the_network_object(gpu_ctx, monkeypatch):
    """At the benchmark's batch sizes the network object takes paths the small-batch tests never reach: the GroupNorm statistics of the bottlenecks' expanding
    convolutions from the input's Gram matrices (csrc/gram.hip: >= 150 M output elements, i.e. >= 31 frames of 480 x 640) and the 256 x 256 GEMM tiles.  48 frames:
    the depth with the Gram statistics is reproducible, equals the Python orchestration bit for bit (same rule there), and is within rounding noise of the two-pass
    statistics (HIVE_GN_GRAM=0) -- which in turn are what the small-batch parity tests pin."""
    from hive_amd import depth as depth_mod
    _, hip = _pair()
    rng = np.random.default_rng(5)
    frames = torch.from_numpy(rng.integers(0, 256, (48, 480, 640, 3), dtype=np.uint8)).cuda()
    with torch.no_grad():
        d_gram, _, _ = hip.forward_frames(frames, max_depth=10.0)
        d_again, _, _ = hip.forward_frames(frames, max_depth=10.0)
        d_py, _, _ = hip(depth_mod.preprocess_on_device(frames[:33], torch.bfloat16), handoff=(10.0,))
        d_c33, _, _ = hip.forward_frames(frames[:33], max_depth=10.0)
        monkeypatch.setenv("HIVE_GN_GRAM", "0")
        d_two, _, _ = hip.forward_frames(frames, max_depth=10.0)
    assert torch.isfinite(d_gram).all() and torch.equal(d_gram, d_again)
    assert torch.equal(d_c33, d_py), "network object and Python orchestration take the same statistics path"
    assert not torch.equal(d_gram, d_two), "48 frames are past the threshold: the Gram path must have been taken"
    # the two forms differ by 16-bit roundings that the rest of the network amplifies (two bfloat16 implementations of this network are ~18 mm apart in the
    # median, smoke()): what counts is that neither is further from the float32 network than the other
    ref, _ = _pair()
    x4 = ((frames[:4].float() / 255.0 - 0.5) / 0.5).permute(0, 3, 1, 2).contiguous()  # (dataset_adaptors.py:1407 + NormalizeImage(0.5, 0.5))
    with torch.no_grad():
        d_ref = ref.cuda()(x4)
    e_gram, e_two = _median_mm(d_gram[:4], d_ref), _median_mm(d_two[:4], d_ref)
    assert e_gram <= 1.15 * e_two + 1.0, (e_gram, e_two)
    assert _median_mm(d_gram, d_two) <= 0.75 * max(e_gram, e_two) + 1.0, (_median_mm(d_gram, d_two), e_gram, e_two)


def test_native_network_object_dpt_large(gpu_ctx):
    """hive_dpt_create(backbone = 1): DPT-Large (vitl16_384) as one C-ABI object -- patch embedding as rows + GEMM, 24 blocks, four
    readouts, ConvTranspose reassembly -- bit-identical to the Python orchestration of the same kernels, at two frame sizes."""
    from dpt_weights import seeded_init
    from hive_amd import depth as depth_mod
    from hive_amd.dpt.models import DPTDepthModel
    ref = DPTDepthModel(path=None, scale=0.000305, shift=0.1378, invert=True, backbone="vitl16_384", engine="hip").eval()
    seeded_init(ref, seed=7)
    hip = ref.to(memory_format=torch.channels_last).to(torch.bfloat16).cuda()
    rng = np.random.default_rng(3)
    for (b, h, w) in ((2, 96, 160), (1, 480, 864)):
        frames = torch.from_numpy(rng.integers(0, 256, (b, h, w, 3), dtype=np.uint8)).cuda()
        with torch.no_grad():
            d_py, mm_py, m_py = hip(depth_mod.preprocess_on_device(frames, torch.bfloat16), handoff=(10.0,))
            d_c, mm_c, m_c = hip.forward_frames(frames, max_depth=10.0)
        assert d_c.shape == (b, h, w) and torch.isfinite(d_c).all()
        assert float(d_c.max() - d_c.min()) > 0.5, "the seeded weights must give a depth range"
        assert torch.equal(d_c, d_py), f"depth differs by up to {float((d_c - d_py).abs().max()) * 1000:.3f} mm"
        assert torch.equal(mm_c, mm_py) and torch.equal(m_c, m_py)


@pytest.mark.parametrize("backbone", ["vitb_rn50_384", "vitl16_384"])
def test_network_object_sizes_its_arena_by_the_exported_plan(gpu_ctx, backbone):
    """A fresh object's arena after one forward is exactly what ``hive_dpt_plan_arena`` answers for that shape (tests/test_dpt_plan_cpu.py pins those
    answers to the recorded layouts): the forward sizes itself by the exported plan, and its launch walk ended at the planned size."""
    from hive_amd.dpt.models import DPTDepthModel
    from hive_amd.dpt.native import NativeDPT
    model = DPTDepthModel(path=None, scale=SCALE, shift=SHIFT, invert=True, engine="hip", backbone=backbone).eval()
    model = model.to(memory_format=torch.channels_last).to(torch.bfloat16).cuda()
    nat = NativeDPT(model, ctx=gpu_ctx)
    assert nat.arena_bytes() == 0
    frames = torch.from_numpy(np.random.default_rng(9).integers(0, 256, (2, 96, 160, 3), dtype=np.uint8)).cuda()
    depth, _, _ = nat.forward(frames, max_depth=10.0)
    assert depth.shape == (2, 96, 160)
    assert nat.arena_bytes() == nat.plan_arena(2, 96, 160) == {"vitb_rn50_384": 8421888, "vitl16_384": 8171520}[backbone]
    nat.close()
