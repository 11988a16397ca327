"""N > 1 path on CPU: two gloo ranks share weights by broadcast and denoise disjoint clips
(the engine runs on the op emulator here; -m gpu covers the kernels)."""
import os
import sys

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _worker(rank, world, port, tmp):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from emu_ops import EmuOps
    from followyourclick_amd import distributed as D
    from followyourclick_amd.engine import DDIMConfig, UNet3DConfig
    from followyourclick_amd.engine.sampler import DDIMSampler
    from followyourclick_amd.engine.schema import random_state_dict, unet_schema
    from followyourclick_amd.engine.unet3d import UNet3DEngine
    from followyourclick_amd.engine.weights import pack_unet
    r, w, _ = D.init_from_env(backend="gloo")
    assert (r, w) == (rank, world)
    cfg = UNet3DConfig(block_out_channels=(64, 128, 256, 256), cross_attention_dim=64, sample_size=8)
    # only rank 0 has real weights; the others start from garbage and must receive the broadcast
    sd = random_state_dict(unet_schema(cfg), seed=0, materialize=True) if rank == 0 else \
        {k: torch.full_like(v, 7.0) for k, v in random_state_dict(unet_schema(cfg), seed=1).items()}
    P = pack_unet(sd, cfg, torch.float32, "cpu")
    moved = D.broadcast_packed(P, src=0, bucket_bytes=1 << 20)
    assert moved > 0
    eng = UNet3DEngine(P, ops=EmuOps())
    n_clips = 3
    mine = D.shard_indices(n_clips, rank, world)
    res = {}
    for i in mine:
        g = torch.Generator().manual_seed(100 + i)
        lat = torch.randn(1, 4, 2, 8, 8, generator=g)
        first = torch.randn(1, 4, 8, 8, generator=g)
        text = torch.randn(2, 77, 64, generator=g)
        res[i] = DDIMSampler(eng, DDIMConfig()).sample(lat, text, 2, 8.0, first, None, fps=[2], flow=[4])
    D.barrier()
    t = D.max_over_ranks(float(rank + 1), "cpu")
    assert t == float(world)
    torch.save({"clips": res, "w": P.conv_in_w.clone(), "temb": P.temb_w[:4].clone()}, os.path.join(tmp, f"rank{rank}.pt"))
    dist.destroy_process_group()


def test_two_ranks_share_weights_and_split_clips(tmp_path):
    world, port = 2, 29741
    mp.spawn(_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    a, b = (torch.load(os.path.join(tmp_path, f"rank{r}.pt")) for r in (0, 1))
    assert torch.equal(a["w"], b["w"]) and torch.equal(a["temb"], b["temb"])        # weights arrived bit-exact
    assert sorted(a["clips"]) == [0, 2] and sorted(b["clips"]) == [1]                 # clip i -> rank i mod world
    # a clip's result does not depend on which rank ran it: recompute clip 1 with rank 0's weights
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from emu_ops import EmuOps
    from followyourclick_amd.engine import DDIMConfig, UNet3DConfig
    from followyourclick_amd.engine.sampler import DDIMSampler
    from followyourclick_amd.engine.schema import random_state_dict, unet_schema
    from followyourclick_amd.engine.unet3d import UNet3DEngine
    from followyourclick_amd.engine.weights import pack_unet
    cfg = UNet3DConfig(block_out_channels=(64, 128, 256, 256), cross_attention_dim=64, sample_size=8)
    eng = UNet3DEngine(pack_unet(random_state_dict(unet_schema(cfg), 0), cfg, torch.float32, "cpu"), ops=EmuOps())
    g = torch.Generator().manual_seed(101)
    lat, first, text = torch.randn(1, 4, 2, 8, 8, generator=g), torch.randn(1, 4, 8, 8, generator=g), torch.randn(2, 77, 64, generator=g)
    ref = DDIMSampler(eng, DDIMConfig()).sample(lat, text, 2, 8.0, first, None, fps=[2], flow=[4])
    assert torch.allclose(ref, b["clips"][1], atol=1e-5)


def test_shard_indices():
    from followyourclick_amd.distributed import shard_indices
    assert [shard_indices(8, r, 8) for r in range(8)] == [[r] for r in range(8)]
    assert shard_indices(5, 1, 2) == [1, 3] and shard_indices(1, 3, 8) == []


def _dropin_worker(rank, world, port, tmp):
    """the drop-in classes themselves: only rank 0 holds the real checkpoint, the others receive the packed tree"""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import followyourclick_amd
    from emu_ops import EmuOps
    from followyourclick_amd import distributed as D
    from followyourclick_amd import ops as ops_mod
    ops_mod.impl = EmuOps()                     # CPU test: host orchestration on the op emulator
    followyourclick_amd.install_dropin(force=True)
    from animatediff.models.unet import UNet3DConditionModel
    from test_dropin_api import TINY
    D.init_from_env(backend="gloo")
    torch.manual_seed(1234 + rank)              # every rank starts from DIFFERENT random parameters
    unet = UNet3DConditionModel(**TINY)
    ckpt = os.path.join(tmp, "unet.pt")
    if rank == 0:
        torch.save(unet.state_dict(), ckpt)
    D.barrier()
    loaded = D.load_on_rank0(unet, lambda: unet.load_state_dict(torch.load(ckpt), strict=False))     # explicit collective: every rank calls it
    assert (loaded is not None) == (rank == 0)
    try:
        D.load_on_rank0(lambda: None)                       # the round-2 call form (no module) must fail loudly, not skip the broadcast
        raise AssertionError("load_on_rank0(loader) without a module was accepted")
    except TypeError:
        pass
    # a loader that fails on rank 0 must fail EVERY rank (a status word precedes the weight broadcast), not leave the others waiting
    def bad_loader():
        raise FileNotFoundError("no such checkpoint")
    try:
        D.load_on_rank0(unet, bad_loader)
        raise AssertionError("a failing loader was swallowed")
    except FileNotFoundError:
        assert rank == 0
    except RuntimeError as e:
        assert rank != 0 and "rank 0" in str(e)
    # anything with a state dict is covered, buffers included (the VAE encoder half, Resampler, ImageProjModel were not in round 2)
    extra = torch.nn.Sequential(torch.nn.Linear(8, 8), torch.nn.BatchNorm1d(8))
    extra[1].running_mean.fill_(float(rank + 1))
    moved = D.broadcast_module(extra)
    assert moved > 0 and float(extra[1].running_mean[0]) == 1.0
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 9, 2, 8, 8, generator=g)
    text = torch.randn(2, 77, 64, generator=g)
    out = unet(x, torch.tensor(500), text, use_fps_condition=True, fps_tensor=torch.tensor([2, 2]), flow_control=torch.tensor([4, 4])).sample
    torch.save({"out": out, "w": unet._engine.P.conv_in_w.clone()}, os.path.join(tmp, f"dropin{rank}.pt"))
    dist.destroy_process_group()


def test_dropin_unet_receives_rank0_weights(tmp_path):
    """scripts/inference.py --ddp equivalent: `load_on_rank0(module, loader)` reads the checkpoint on rank 0 and broadcasts the
    module's state dict, so the ranks that never read the checkpoint produce rank 0's outputs; nothing collective is hidden in
    the forward any more (round-2 advice: the lazy broadcast covered only part of the modules and could deadlock)"""
    world, port = 2, 29743
    mp.spawn(_dropin_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    a, b = (torch.load(os.path.join(tmp_path, f"dropin{r}.pt")) for r in (0, 1))
    assert torch.equal(a["w"], b["w"])
    assert torch.equal(a["out"], b["out"])


def test_bench_entry_point_under_torch_distributed_run(tmp_path):
    """bench.py as the driver launches it for N > 1 (`python -m torch.distributed.run --nproc-per-node 2 ... bench.py --gpus 2`):
    rendezvous on 127.0.0.1, weight broadcast, per-rank clips, barrier + max-over-ranks timing, ONE JSON line from rank 0 -
    with gloo and the op emulator injected by the tests-side wrapper tests/bench_emulated.py (bench.main(emulation=...); the line
    says "data": "emulated"; labels follow the arguments).  No RCCL run of this
    path exists yet (SCALE_rNN.json has been a skip record): this keeps the launch path from failing first on an 8-GPU node."""
    import json
    import subprocess
    env = dict(os.environ, OMP_NUM_THREADS="2")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", "29771",
           os.path.join(ROOT, "tests", "bench_emulated.py"), "--gpus", "2", "--steps", "1", "--warmup", "1", "--frames", "2", "--size", "64", "--ddim-steps", "2", "--dtype", "f32",
           "--full"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 1 and d["warmup"] == 1 and d["scaling"] == "weak" and d["data"] == "emulated"
    assert d["value"] > 0 and abs(d["value"] - 2 * 2 * 1 / (d["ms_per_step"] / 1000.0)) / d["value"] < 1e-2      # whole-job frames/s = n * frames * K / max time
    assert d["host_launch_ms_per_ddim_step"] > 0 and "parallelism" in d["config"] and d["config"]["parallelism"].startswith("dp2")
    assert d["metric"] == "denoised frames/sec, 2f x 64^2 clip @ 2 DDIM steps" and d["config"]["workload"].startswith("custom")


def test_bench_plain_invocation_launches_its_own_ranks(tmp_path):
    """`python bench.py --gpus 2` with NO launcher around it (the form a driver may use for the scaling run): the script re-executes
    itself under torch.distributed.run and the line says n_gpus 2 with 2 ranks counted by an all-reduce - never a silent N = 1
    (round-4 review).  A launcher that starts a different number of ranks than --gpus is an error, not an override."""
    import json
    import subprocess
    env = dict(os.environ, OMP_NUM_THREADS="2")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "TORCHELASTIC_RUN_ID"):
        env.pop(k, None)
    tail = ["--steps", "1", "--warmup", "1", "--frames", "2", "--size", "64", "--ddim-steps", "2", "--dtype", "f32"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "bench_emulated.py"), "--gpus", "2", *tail], env=env, capture_output=True, text=True,
                       timeout=900, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["rccl_ranks"] == 2 and d["collective_backend"] == "gloo" and d["data"] == "emulated"
    # one rank started for a 2-GPU request: non-zero exit, no JSON line
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1", "--master-port", "29773",
           os.path.join(ROOT, "tests", "bench_emulated.py"), "--gpus", "2", *tail]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=str(tmp_path))
    assert r.returncode != 0
    assert not [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert "refusing" in r.stderr


def test_bench_plain_run_dumps_reproducible_outputs(tmp_path):
    """a plain run (no --full) prints the headline fields only and, with --dump-outputs, writes the last timed clip's latents; the
    inputs are seeded, so two runs with the same arguments dump the same array"""
    import json
    import subprocess
    import numpy as np
    env = dict(os.environ, OMP_NUM_THREADS="2")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "TORCHELASTIC_RUN_ID"):
        env.pop(k, None)
    dumps = []
    for run in ("a", "b"):
        out = tmp_path / run
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "bench_emulated.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--frames", "2",
                            "--size", "64", "--ddim-steps", "2", "--dtype", "f32", "--dump-outputs", str(out)],
                           env=env, capture_output=True, text=True, timeout=900, cwd=str(tmp_path))
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, r.stdout[-2000:]
        d = json.loads(lines[0])
        assert d["steps"] == 2 and d["ms_per_step"] > 0 and d["unit"] == "frames/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
        assert "host_launch_ms_per_ddim_step" not in d
        assert sorted(os.listdir(out)) == ["latents.npy"]
        dumps.append(np.load(out / "latents.npy"))
    assert dumps[0].dtype == np.float32 and dumps[0].shape == (1, 4, 2, 8, 8)
    assert np.array_equal(dumps[0], dumps[1])


def test_bench_labels_follow_the_arguments():
    """only the default arguments claim BASELINE.json's configs[1] (round 3 stamped every line with it)"""
    import argparse
    import bench
    ns = lambda **kw: argparse.Namespace(**kw)   # noqa: E731
    assert bench.workload_label(ns(frames=16, size=512, ddim_steps=25, ip_tokens=0)) == "configs[1]"
    assert bench.workload_label(ns(frames=16, size=512, ddim_steps=25, ip_tokens=0, dtype="f16")) == "configs[1] at f16 instead of the config's bf16"
    assert bench.workload_label(ns(frames=8, size=256, ddim_steps=5, ip_tokens=0)) == "configs[0]"
    assert bench.workload_label(ns(frames=32, size=768, ddim_steps=50, ip_tokens=0)) == "configs[3]"
    assert bench.workload_label(ns(frames=16, size=512, ddim_steps=25, ip_tokens=16)) == "configs[4]"
    assert bench.workload_label(ns(frames=16, size=512, ddim_steps=2, ip_tokens=0)).startswith("custom")
    cores, logical = bench.numa_node_cores(0)
    assert 1 <= len(cores) <= logical


def test_bench_helper_legs_fail_soft_and_traffic_matches_by_family():
    """the extra legs of the bench line never cost the line: a reference CPU run that does not finish in time hands over to the port
    (None + a reason), a missing staged tree likewise; and `roofline.traffic` is matched per kernel family - the committed PMC profile of the
    GEMM family stays valid when another family's source changed afterwards (followyourclick_amd/_build.py::family_digest)"""
    import glob
    import json
    import bench
    from followyourclick_amd import _build
    d, why = bench.cpu_baseline_reference(2, 64, 2, 1, timeout_s=1)
    assert d is None and ("did not finish" in why or "not staged" in why)
    fam = _build.family_digest("gemm")
    assert fam == _build.family_digest("gemm") and len(fam) == 64
    newest = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_hbm_traffic.json")), reverse=True)[0]
    doc = json.load(open(newest))
    assert doc.get("gemm_family_source_sha256") == fam, "the GEMM-family sources changed after the newest PMC traffic profile was taken: re-run tools/collect_profiles.sh"
    assert doc["families"]["gemm"]["hbm_bytes_per_launch"] > 1e8
