"""Two ranks (gloo control plane, both on cuda:0 of the one-GPU box) run the sharded Flow pipeline on a
halo-split clip; outputs and meta must equal the single-process result bit for bit."""

import json
import os
import socket
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]


def _clip():
    from tests.test_dis_gpu import moving_clip

    gray, _ = moving_clip(9, 270, 480, seed=5)
    f = np.repeat(gray[..., None].astype(np.float32) / 255.0, 3, axis=-1)
    f[..., 2] = 1.0 - f[..., 2]
    return np.ascontiguousarray(f)


def _worker(rank, world, port, out_dir, estimator, framing="expand", keep_fov=0.6, n_frames=9, backend="gloo"):
    sys.path.insert(0, str(ROOT))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch
    import torch.distributed as dist

    import __graft_entry__ as graft

    graft.load_package()
    from vstab_amd import distributed as vd
    from vstab_amd import native

    torch.cuda.set_device(0)
    if backend == "nccl":
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", 0))
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        ctx = native.Context(0)
        frames = _clip()[:n_frames]
        n = frames.shape[0]
        start, end = vd.shard_range(n, world, rank)
        halo = 1 if (rank > 0 and end > start) else 0
        local = torch.from_numpy(frames[start - halo:end]).cuda()
        stats = {}
        dst, mask, meta = vd.stabilize_sharded(ctx, local, n, framing, "similarity", False, 0.7, 0.5, keep_fov, (127, 127, 127), 16.0,
                                               estimator=estimator, stats=stats)
        np.save(Path(out_dir) / f"dst_{rank}.npy", dst.cpu().numpy())
        np.save(Path(out_dir) / f"mask_{rank}.npy", mask.cpu().numpy())
        (Path(out_dir) / f"meta_{rank}.json").write_text(json.dumps(meta))
        (Path(out_dir) / f"device_plan_{rank}.json").write_text(json.dumps(stats.get("device_plan")))
        if backend == "nccl":   # the replay half of BASELINE C5 under the same process group (it issues no collective)
            from vstab_amd import apply_pipeline as ap

            own = torch.from_numpy(frames[start:end]).cuda()
            a_dst, a_mask, a_meta = vd.apply_motion_sharded(ctx, own, start, n, meta, (127, 127, 127), framing_mode="expand",
                                                            interpolation="bilinear", motion_blur=0.5, motion_blur_samples=33)
            np.save(Path(out_dir) / f"apply_dst_{rank}.npy", a_dst.cpu().numpy())
            np.save(Path(out_dir) / f"apply_mask_{rank}.npy", a_mask.cpu().numpy())
            (Path(out_dir) / f"apply_meta_{rank}.json").write_text(json.dumps(a_meta))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("estimator", ["flow", "classic", "flow_phase_correlate"])
def test_two_rank_shards_equal_single_process(pkg, ctx, tmp_path, estimator):
    from vstab_amd import flow_pipeline as fp
    from vstab_amd import host_math as hm

    _spawn(2, tmp_path, estimator)
    frames = _clip()
    ref = fp._stabilize_frames(hm._normalize_video_input(frames), "expand", "similarity", False, 0.7, 0.5, 0.6, (127, 127, 127), 16.0,
                               estimator=estimator)
    dst = np.concatenate([np.load(tmp_path / f"dst_{r}.npy") for r in range(2)])
    mask = np.concatenate([np.load(tmp_path / f"mask_{r}.npy") for r in range(2)])
    assert np.array_equal(dst, ref.frames) and np.array_equal(mask, ref.masks[..., 0])
    want = json.loads(json.dumps(ref.meta))
    for r in range(2):
        assert json.loads((tmp_path / f"meta_{r}.json").read_text()) == want


def _spawn(world, tmp_path, *extra):
    import torch.multiprocessing as mp

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_worker, args=(world, port, str(tmp_path)) + extra, nprocs=world, join=True)


def test_sharded_device_plan_under_rccl_equals_single_process(pkg, ctx, tmp_path):
    """The speculative device plan of the sharded path (distributed._stabilize_sharded_device_plan: fit records device ->
    all_gather_into_tensor -> plan_kernel on the gathered table -> warp, host plan + verification meanwhile) inside a real
    "nccl" group (a world of one: RCCL refuses two ranks on one device), crop_and_pad + similarity = the C4 configuration;
    equal to the single-process node bit for bit, and the speculation was taken with no frame warped twice."""
    from vstab_amd import flow_pipeline as fp
    from vstab_amd import host_math as hm

    _spawn(1, tmp_path, "flow", "crop_and_pad", 0.6, 9, "nccl")
    frames = _clip()
    ref = fp._stabilize_frames(hm._normalize_video_input(frames), "crop_and_pad", "similarity", False, 0.7, 0.5, 0.6, (127, 127, 127), 16.0)
    assert json.loads((tmp_path / "device_plan_0.json").read_text()) == {"used": True, "mismatched_frames": 0}
    assert np.array_equal(np.load(tmp_path / "dst_0.npy"), ref.frames) and np.array_equal(np.load(tmp_path / "mask_0.npy"), ref.masks[..., 0])
    assert json.loads((tmp_path / "meta_0.json").read_text()) == json.loads(json.dumps(ref.meta))


@pytest.mark.parametrize("world,n_frames,framing", [(2, 9, "crop_and_pad"), (3, 9, "crop_and_pad"), (3, 2, "crop_and_pad"),
                                                    (2, 9, "expand"), (3, 2, "expand")])
def test_sharded_device_plan_with_several_ranks_equals_single_process(pkg, ctx, tmp_path, monkeypatch, world, n_frames, framing):
    """The multi-rank layout of the device-plan form -- every rank's records into its row block of the gathered table,
    plan_kernel on that table through the segment table, each rank's warp from ITS slice of the device plan, the host plan's
    verification of that slice, a rank without frames (3 ranks, 2 frames), the expand framing (every rank sizes the canvas from
    its own copy of the plan kernel's region) -- with real ranks on the one GPU
    (VSTAB_SHARDED_DEVICE_PLAN=force: gloo control plane, the collectives through the host).  Equal to the single-process
    node bit for bit on every rank."""
    from vstab_amd import flow_pipeline as fp
    from vstab_amd import host_math as hm

    monkeypatch.setenv("VSTAB_SHARDED_DEVICE_PLAN", "force")
    _spawn(world, tmp_path, "flow", framing, 0.6, n_frames)
    frames = _clip()[:n_frames]
    ref = fp._stabilize_frames(hm._normalize_video_input(frames), framing, "similarity", False, 0.7, 0.5, 0.6, (127, 127, 127), 16.0)
    dst = np.concatenate([np.load(tmp_path / f"dst_{r}.npy") for r in range(world)])
    mask = np.concatenate([np.load(tmp_path / f"mask_{r}.npy") for r in range(world)])
    assert np.array_equal(dst, ref.frames) and np.array_equal(mask, ref.masks[..., 0])
    want = json.loads(json.dumps(ref.meta))
    for r in range(world):
        assert json.loads((tmp_path / f"meta_{r}.json").read_text()) == want
        assert json.loads((tmp_path / f"device_plan_{r}.json").read_text()) == {"used": True, "mismatched_frames": 0}


def test_rccl_branches_run_with_a_world_of_one(pkg, ctx, tmp_path):
    """VERDICT r2 #3c / ADVICE r2: the RCCL-only code of distributed.py -- `all_gather_into_tensor` on DEVICE tensors for
    the fit records (`_gather_rows`, nccl branch) and for the int32 padded-pixel counts the warp kernel filled
    (`_start_gather_counts(on_device=True)`, enqueued stream-ordered behind the kernel) -- inside a real "nccl" process
    group.  One GPU holds one rank (RCCL refuses two ranks on a device), so the group has a world of one, started as a
    child process; results must equal the single-process pipeline bit for bit, Flow (expand) and the Motion Apply replay
    (expand, bilinear, blur 0.5, 33 samples: BASELINE C5's chain) alike."""
    from vstab_amd import apply_pipeline as ap
    from vstab_amd import flow_pipeline as fp
    from vstab_amd import host_math as hm

    _spawn(1, tmp_path, "flow", "expand", 0.6, 9, "nccl")
    frames = _clip()
    ref = fp._stabilize_frames(hm._normalize_video_input(frames), "expand", "similarity", False, 0.7, 0.5, 0.6, (127, 127, 127), 16.0)
    assert np.array_equal(np.load(tmp_path / "dst_0.npy"), ref.frames) and np.array_equal(np.load(tmp_path / "mask_0.npy"), ref.masks[..., 0])
    assert json.loads((tmp_path / "meta_0.json").read_text()) == json.loads(json.dumps(ref.meta))
    replay = ap.apply_motion(hm._normalize_video_input(frames), ref.meta, (127, 127, 127), framing_mode="expand", interpolation="bilinear",
                             motion_blur=0.5, motion_blur_samples=33)
    assert np.array_equal(np.load(tmp_path / "apply_dst_0.npy"), replay.frames)
    assert np.array_equal(np.load(tmp_path / "apply_mask_0.npy"), replay.masks[..., 0])
    assert json.loads((tmp_path / "apply_meta_0.json").read_text()) == json.loads(json.dumps(replay.meta))


def test_rank_without_frames_does_not_hang(pkg, ctx, tmp_path):
    """total_frames < world left a rank with n_local == 0, whose warp call raised on that rank only
    while the others blocked in the second all-gather.  3 ranks, 2 frames: rank 2 owns nothing, still joins both
    collectives, and the concatenated result equals the single-process one."""
    from vstab_amd import flow_pipeline as fp
    from vstab_amd import host_math as hm

    _spawn(3, tmp_path, "flow", "crop_and_pad", 0.6, 2)
    frames = _clip()[:2]
    ref = fp._stabilize_frames(hm._normalize_video_input(frames), "crop_and_pad", "similarity", False, 0.7, 0.5, 0.6,
                               (127, 127, 127), 16.0)
    parts = [np.load(tmp_path / f"dst_{r}.npy") for r in range(3)]
    assert [p.shape[0] for p in parts] == [1, 1, 0]
    assert np.array_equal(np.concatenate(parts), ref.frames)
    want = json.loads(json.dumps(ref.meta))
    for r in range(3):
        assert json.loads((tmp_path / f"meta_{r}.json").read_text()) == want


def test_sharded_crop_bypass_returns_own_frames(pkg, ctx, tmp_path):
    """flow.py:387-429 through the sharded driver (was NotImplementedError in round 1): crop + keep_fov 1.0 hands
    back the original frames, zero masks and the bypass meta, identical to the single-process path."""
    from vstab_amd import flow_pipeline as fp
    from vstab_amd import host_math as hm

    _spawn(2, tmp_path, "flow", "crop", 1.0, 9)
    frames = _clip()
    ref = fp._stabilize_frames(hm._normalize_video_input(frames), "crop", "similarity", False, 0.7, 0.5, 1.0, (127, 127, 127), 16.0)
    dst = np.concatenate([np.load(tmp_path / f"dst_{r}.npy") for r in range(2)])
    mask = np.concatenate([np.load(tmp_path / f"mask_{r}.npy") for r in range(2)])
    assert np.array_equal(dst, frames) and np.array_equal(dst, ref.frames) and not mask.any()
    want = json.loads(json.dumps(ref.meta))
    assert want["note"].startswith("keep_fov~=1.0")
    for r in range(2):
        assert json.loads((tmp_path / f"meta_{r}.json").read_text()) == want


@pytest.mark.parametrize("framing,interp,blur,samples", [("expand", "bilinear", 0.5, 33), ("crop_and_pad", "bicubic", 0.5, 17),
                                                         ("crop", "bilinear", 0.3, 5), ("expand", "bicubic", 0.0, 9)])
@pytest.mark.parametrize("world", [2, 3])
def test_sharded_motion_apply_equals_single_process(pkg, ctx, framing, interp, blur, samples, world):
    """BASELINE config C5's missing piece: Motion Apply over frame shards.  No process group is involved
    -- the path has no collective -- so the shards are replayed one after the other on this GPU: their concatenation
    must equal apply_motion on the whole clip bit for bit, including the blurred frames at the shard edges (whose
    sample delta uses the neighbour rank's matrix, motion_apply.py:125-134) and the clip's last frame (backward delta),
    the expand canvas and the crop matrix (clip-global), and the result meta."""
    import torch

    from vstab_amd import apply_pipeline as ap
    from vstab_amd import distributed as vd
    from vstab_amd import host_math as hm
    from vstab_amd import meta_v2 as mv
    from tests.util import synth_frames, test_matrices

    n, h, w = 7, 90, 120
    frames = synth_frames(n, h, w, seed=3)
    mats = test_matrices(n, w, h, "perspective" if framing != "crop" else "translation", seed=11)
    if framing == "crop":
        mats = [np.array([[1, 0, 0.6 * m[0, 2]], [0, 1, 0.6 * m[1, 2]], [0, 0, 1.0]]) for m in mats]
    meta = {"motion_meta": mv.build_motion_meta_v2(source="manual", frame_count=n, fps=16.0, input_size=(w, h), output_size=(w, h),
                                                   matrices=list(mats))}
    kw = dict(framing_mode=framing, interpolation=interp, motion_blur=blur, motion_blur_samples=samples)
    ticks_ref = []
    ref = ap.apply_motion(hm._normalize_video_input(frames), meta, (10, 200, 30), progress_callback=lambda: ticks_ref.append(1), **kw)
    parts, masks, ticks = [], [], []
    for rank in range(world):
        s, e = vd.shard_range(n, world, rank)
        f, m, rmeta = vd.apply_motion_sharded(ctx, torch.from_numpy(frames[s:e]).cuda(), s, n, meta, (10, 200, 30),
                                              progress_callback=lambda: ticks.append(1), **kw)
        parts.append(f.cpu().numpy())
        masks.append(m.cpu().numpy())
        assert json.loads(json.dumps(rmeta)) == json.loads(json.dumps(ref.meta))
    assert np.array_equal(np.concatenate(parts), ref.frames)
    assert np.array_equal(np.concatenate(masks), ref.masks[..., 0])
    assert len(ticks) == len(ticks_ref)
    if framing == "crop":
        assert "framing_fallback" not in ref.meta and not ref.masks.any()
    # an empty shard (clip shorter than the world) yields empty tensors of the right geometry and the same meta
    f, m, rmeta = vd.apply_motion_sharded(ctx, torch.from_numpy(frames[n:n]).cuda(), n, n, meta, (10, 200, 30), **kw)
    assert f.shape[0] == 0 and tuple(f.shape[1:]) == ref.frames.shape[1:] and json.loads(json.dumps(rmeta)) == json.loads(json.dumps(ref.meta))
    with pytest.raises(ValueError, match="Frame count mismatch"):
        vd.apply_motion_sharded(ctx, torch.from_numpy(frames[:3]).cuda(), 0, n + 1, meta, (10, 200, 30), **kw)


def _c4_worker(rank, world, port, out_dir, total, h, w):
    """One rank of the C4-sized run: synthesises ITS shard of the bench clip on the GPU (halo frame included), runs the
    sharded Flow pipeline, leaves per-frame bit checksums, three whole frames and the meta behind."""
    sys.path.insert(0, str(ROOT))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch
    import torch.distributed as dist

    import __graft_entry__ as graft

    graft.load_package()
    import bench
    from vstab_amd import distributed as vd
    from vstab_amd import native

    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        ctx = native.Context(0)
        start, end = vd.shard_range(total, world, rank)
        halo = 1 if rank > 0 else 0
        local = bench.synth_clip(end - start + halo, start - halo, h, w, torch.device("cuda", 0))
        dst, mask, meta = vd.stabilize_sharded(ctx, local, total, *bench.FLOW_ARGS)
        torch.save({"dst": _frame_checksums(dst), "mask": _frame_checksums(mask), "start": start,
                    "frames": {i: dst[i - start].cpu() for i in (start, (start + end) // 2, end - 1)}},
                   Path(out_dir) / f"c4_{rank}.pt")
        if rank == 0:
            (Path(out_dir) / "c4_meta.json").write_text(json.dumps(meta))
    finally:
        dist.destroy_process_group()


def _frame_checksums(t):
    """Order-independent exact checksum per frame: the float bit patterns summed as int64."""
    import torch

    return t.contiguous().view(torch.int32).reshape(t.shape[0], -1).to(torch.int64).sum(dim=1).cpu()


def test_c4_sized_clip_two_ranks_equal_single_process(pkg, ctx, tmp_path):
    """BASELINE configs[3] at its SIZE: one 1024-frame 1080p clip, Flow similarity + crop_and_pad,
    sharded over two ranks (both on this box's one GPU, gloo control plane -- RCCL refuses two ranks on a device), against
    the single-process pipeline on the same 1024 frames: per-frame bit checksums of every output frame and mask, three
    whole frames per rank and the whole meta (plan over 1023 transitions, halo pair at frame 512) must be equal.  The
    single-process path is the one checked against the oracle at 256 frames (tests/test_configs_gpu.py)."""
    import torch
    import torch.multiprocessing as mp

    import bench
    from vstab_amd import flow_pipeline as fp
    from vstab_amd import host_math as hm

    total, h, w = 1024, 1080, 1920
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_c4_worker, args=(2, port, str(tmp_path), total, h, w), nprocs=2, join=True)
    frames = bench.synth_clip(total, 0, h, w, torch.device("cuda", 0))
    res = fp._stabilize_frames(hm._normalize_video_input(frames), *bench.FLOW_ARGS, ctx=ctx, keep_on_device=True)
    del frames
    # the single-process side ran on the device-formed plan (the two ranks above form theirs on the host) and none of the
    # 1024 device matrices differed from the host's: the equality below is the speculation holding, not its fallback
    assert res.device_plan == {"used": True, "mismatched_frames": 0}
    want_dst, want_mask = _frame_checksums(res.frames), _frame_checksums(res.masks)
    parts = [torch.load(tmp_path / f"c4_{r}.pt") for r in range(2)]
    assert [p["start"] for p in parts] == [0, 512]
    assert torch.equal(torch.cat([p["dst"] for p in parts]), want_dst)
    assert torch.equal(torch.cat([p["mask"] for p in parts]), want_mask)
    for p in parts:
        for i, f in p["frames"].items():
            assert torch.equal(f, res.frames[i].cpu()), i
    assert json.loads((tmp_path / "c4_meta.json").read_text()) == json.loads(json.dumps(res.meta))
    assert res.meta["frames"] == total and len(res.meta["estimated_motion"]["per_transition"]) == total - 1


def test_bench_default_multi_rank_line_rehearsed_on_one_gpu():
    """`bench.py --gpus 2 --full` as the driver's scaling run starts it, except that both ranks share this box's GPU (gloo control
    plane, `--rehearse-on-one-gpu`): the child launcher, the default workload (the metric's 256 frames per GPU as one 512-frame clip,
    weak scaling), the `c4` object (BASELINE configs[3], strong scaling, with the same clip's one-GPU record) and the `c5` object all
    have to produce their part of the ONE JSON line.  The numbers mean nothing here; the structure is what a multi-GPU run prints."""
    root = ROOT
    proc = subprocess.run([sys.executable, str(root / "bench.py"), "--gpus", "2", "--rehearse-on-one-gpu", "--steps", "1", "--warmup", "1",
                           "--c5-frames", "4", "--full"], capture_output=True, text=True, timeout=600, cwd=str(root))
    assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-4000:]
    lines = [ln for ln in proc.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, proc.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["scaling"] == "weak" and line["metric"] == "stabilized frames/sec (1080p, similarity mode)"
    assert line["config"]["total_frames"] == 512 and line["config"]["frames_per_gpu"] == 256 and "rehearsal" in line["config"]
    assert line["value"] > 0 and abs(line["value"] - 512 / (line["ms_per_step"] * 1e-3)) <= 0.01 * line["value"]
    assert line["roofline"]["algorithmic_bytes_per_launch"] == 28 * 1920 * 1080 * 256 and "cpu_baseline" not in line
    c4 = line["c4"]
    assert "error" not in c4 and c4["scaling"] == "strong" and c4["frames_per_gpu"] == 512 and c4["value"] > 0
    assert c4["same_clip_on_one_gpu"]["ms_per_step"] > 0 and "rank0_host_ms" in c4
    c5 = line["c5"]
    assert "error" not in c5 and c5["total_frames"] == 4 and c5["n_gpus"] == 2 and c5["value"] > 0


def test_bench_plain_line_and_dumped_outputs(tmp_path):
    """A plain `bench.py --gpus 1` run (no --full) prints the headline line without the extras, and `--dump-outputs DIR`
    writes what its last timed step returned as float32 / float64 .npy files within 64 MB; two runs with the same arguments
    write the same values (the clip is synthesised from fixed seeds and the path is deterministic)."""
    dumps = []
    for k in range(2):
        out_dir = tmp_path / f"run{k}"
        proc = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--frames", "8",
                               "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=300, cwd=str(ROOT))
        assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-4000:]
        lines = [ln for ln in proc.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, proc.stdout[-2000:]
        line = json.loads(lines[0])
        assert line["metric"] == "stabilized frames/sec (1080p, similarity mode)" and line["unit"] == "frames/s"
        assert line["higher_is_better"] is True and line["dtype"] == "f32" and line["steps"] == 2
        assert line["value"] > 0 and abs(line["value"] - 8 / (line["ms_per_step"] * 1e-3)) <= 0.01 * line["value"]
        for key in ("cpu_baseline", "accuracy", "batch_invariance", "parity_at_size", "host_roundtrip", "motion_apply", "c4", "c5"):
            assert key not in line, key
        assert set(line["config"]["stage_ms"]) == {"warp"} and line["config"]["dis_ms"] is None
        files = sorted(out_dir.glob("*.npy"))
        assert sum(p.stat().st_size for p in files) <= 64 << 20
        arrays = {p.stem: np.load(p) for p in files}
        assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
        assert arrays["frames"].shape[1] == 3 and arrays["masks"].shape == (arrays["frames"].shape[0], 1)
        assert arrays["transition_matrices"].shape == (7, 3, 3) and arrays["applied_matrices"].shape == (8, 3, 3)
        dumps.append(arrays)
    assert set(dumps[0]) == set(dumps[1])
    for name in dumps[0]:
        assert np.array_equal(dumps[0][name], dumps[1][name]), name


def _failing_worker(rank, world, port, out_dir, where, form):
    """Both ranks on cuda:0 (gloo control plane).  After one clean call, rank 1 alone fails at `where`; every rank must come
    out of stabilize_sharded with a ShardError naming rank 1, quickly, and the next clean call must work again."""
    sys.path.insert(0, str(ROOT))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    if form == "device_plan":
        os.environ["VSTAB_SHARDED_DEVICE_PLAN"] = "force"
    import datetime
    import time

    import torch
    import torch.distributed as dist

    import __graft_entry__ as graft

    graft.load_package()
    from vstab_amd import distributed as vd
    from vstab_amd import native

    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    try:
        ctx = native.Context(0)
        frames = _clip()
        n = frames.shape[0]
        start, end = vd.shard_range(n, world, rank)
        halo = 1 if (rank > 0 and end > start) else 0
        local = torch.from_numpy(frames[start - halo:end]).cuda()
        args = (ctx, local, n, "crop_and_pad", "similarity", False, 0.7, 0.5, 0.6, (127, 127, 127), 16.0)
        clean = vd.stabilize_sharded(*args)
        out = {"form_taken": None}
        if rank == 1:   # the injected failure: an exception out of one library call of this rank only
            target = {"estimate": "dis_flow_batch", "fit_end": "sample_fit_batch_end" if form == "device_plan" else "sample_fit_batch",
                      "warp": "warp_batch_planned" if form == "device_plan" else "warp_batch"}[where]
            real = getattr(ctx, target)

            def boom(*a, **k):
                raise native.VstabError(f"injected failure in {target}")

            setattr(ctx, target, boom)
        t0 = time.perf_counter()
        try:
            vd.stabilize_sharded(*args)
            out["error"] = None
        except vd.ShardError as exc:
            out["error"] = {"failed": exc.failed, "text": str(exc)}
        out["seconds"] = time.perf_counter() - t0
        if rank == 1:
            setattr(ctx, target, real)
        stats = {}
        again = vd.stabilize_sharded(*args, stats=stats)
        out["form_taken"] = stats["device_plan"]["used"]
        out["again_equal"] = bool(torch.equal(again[0], clean[0]) and torch.equal(again[1], clean[1]) and again[2] == clean[2])
        (Path(out_dir) / f"failing_{rank}.json").write_text(json.dumps(out))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("form,where", [("host_plan", "estimate"), ("host_plan", "warp"), ("device_plan", "estimate"),
                                        ("device_plan", "fit_end"), ("device_plan", "warp")])
def test_a_rank_that_fails_alone_fails_every_rank_and_nobody_hangs(pkg, ctx, tmp_path, monkeypatch, form, where):
    """`sample_fit_batch_end` (DIS status), the estimation or the warp raising on ONE rank used to leave
    the peers in a collective until the process group's timeout.  The status row / status word that now travels with the two
    all-gathers makes every rank raise the same ShardError -- in both forms of the sharded path, before the first collective
    (reported through it) and between the two (reported through the second) -- within seconds, and the group stays usable."""
    import torch.multiprocessing as mp

    if form == "host_plan":
        monkeypatch.setenv("VSTAB_DEVICE_PLAN", "0")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_failing_worker, args=(2, port, str(tmp_path), where, form), nprocs=2, join=True)
    for rank in range(2):
        out = json.loads((tmp_path / f"failing_{rank}.json").read_text())
        assert out["error"] is not None, out
        assert [r for r, _ in out["error"]["failed"]] == [1], out
        assert out["seconds"] < 5.0, out
        assert out["again_equal"] and out["form_taken"] == (form == "device_plan")
        if where == "estimate":   # reported through the fit-record exchange, with the text
            assert "injected failure in dis_flow_batch" in out["error"]["failed"][0][1]
            assert "before the exchange" in out["error"]["text"]
        else:
            assert "between its two collectives" in out["error"]["text"]
    own = json.loads((tmp_path / "failing_1.json").read_text())["error"]["failed"][0][1]
    assert "injected failure" in own
