#!/usr/bin/env python3
"""Training entry point: the reference's ``train.py`` (``__main__`` at :325-476, loop at :21-322) on the MI355X path.

Same flags, same log lines, same checkpoint format; one process per GPU:

    python train.py --exp_name e0 --dataset_path /data/ffhq --dataset_type normal --num_iters 80000 --batch_size 32
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 train.py ... (batch_size is per GPU)

What differs from the reference: the data loader hands uint8 images to the device and the transform runs
there (ideas_amd/data.py); gradients are averaged across ranks by one RCCL all-reduce per optimiser group (ideas_amd/ddp.py);
Adam + EMA are one fused launch per group (ideas_amd/optim.py); the sample sheet of train.py:293-303 is laid out and written by
ideas_amd.utils.save_image_grid (torchvision is not a dependency).  Below 256x256 the co-occurrence discriminator cannot run (models.py:400);
``--no_dco`` trains without its terms, which is only meant for smoke runs.
"""
import argparse
import os
import random
import time

import torch
import torch.distributed as dist


def time_change(t: float) -> str:
    """utils.py:12-34: '1h 2m 3s' / '2m 3s' / '3s' (thresholds strictly greater than one hour / one minute)."""
    if t / 3600 > 1:
        h = int(t / 3600)
        m = int((t - h * 3600) / 60)
        return f"{h}h {m}m {int(t - h * 3600 - m * 60)}s"
    if t / 60 > 1:
        m = int(t / 60)
        return f"{m}m {int(t - m * 60)}s"
    return f"{int(t)}s"


def main():
    p = argparse.ArgumentParser()
    # the reference's flags (train.py:331-367): name, type, default (None = required)
    for name, typ, default in (("exp_name", str, None), ("dataset_path", str, None), ("num_iters", int, None),
                               ("N", int, 1), ("lambda_Ex", float, 10), ("ckpt", str, ""), ("lr", float, 0.002),
                               ("batch_size", int, 1), ("image_size", int, 256), ("real_r1", float, 10),
                               ("texture_r1", float, 1), ("dist_r1", float, 1), ("ref_crop", int, 4), ("n_crop", int, 8),
                               ("d_reg_every", int, 16), ("channel", int, 32), ("channel_multiplier", int, 1),
                               ("structure_channel", int, 8), ("texture_channel", int, 2048), ("log_every", int, 200),
                               ("show_every", int, 1000), ("save_every", int, 200000)):
        if default is None:
            p.add_argument("--" + name, type=typ, required=True)
        else:
            p.add_argument("--" + name, type=typ, default=default)
    p.add_argument("--dataset_type", choices=["lmdb", "normal"], required=True)
    # additions of this build
    p.add_argument("--no_dco", action="store_true", help="drop the co-occurrence discriminator terms (image_size < 256)")
    p.add_argument("--num_workers", type=int, default=4)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--path_regularize", type=float, default=0.0, help="stylegan2/train.py's lazy path-length weight (off in IDEAS)")
    p.add_argument("--precision", choices=["f32", "bf16"], default="f32",
                   help="f32 = the reference's arithmetic (default); bf16 = mixed precision (bf16 activations and MFMA products, f32 "
                        "accumulation, master weights, gradients and optimiser state: ideas_amd/precision.py, BASELINE.json configs[4])")
    args = p.parse_args()
    args.start_iter = 0
    args.blur_kernel = (1, 3, 3, 1)
    args.use_dco = not args.no_dco
    args.elide_second_backward, args.share_forward = True, True
    args.g_reg_every, args.path_batch_shrink = 4, 2

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("train.py needs an MI355X: the product path has no CPU fallback")
    if os.environ.get("IDEAS_BENCH_SHARE_GPU") == "1":     # test affordance: several ranks on a 1-GPU box (with gloo)
        local_rank = 0
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    if world > 1:
        backend = os.environ.get("IDEAS_DIST_BACKEND", "nccl")          # "nccl" is RCCL on ROCm
        if backend == "nccl":
            # NO device_id: binding the group to the device makes ProcessGroupNCCL create its communicator eagerly, and on this stack
            # (torch 2.10 + RCCL 2.26) every later iteration is then 13.5 ms slower WITHOUT a single collective being issued (f32 393.3 ->
            # 406.9 ms, same box; tools/probes/pg_init_overhead.py, profiles/r06_pg_init_overhead.txt); the lazily created communicator
            # (first collective on the current device, which set_device fixed above) costs nothing (392.9 ms)
            dist.init_process_group(backend="nccl", init_method="env://")
        else:
            dist.init_process_group(backend=backend, init_method="env://")

    from ideas_amd import checkpoint, data as D, precision, train_step as TS
    from ideas_amd.ddp import GradReducer, broadcast_parameters
    from ideas_amd.models import init_model
    from ideas_amd.optim import fuse_optimizers

    base_dir = f"experiments/{args.exp_name}"
    ckpt_dir = f"{base_dir}/checkpoints"
    sample_dir = f"{base_dir}/samples"
    if rank == 0:
        os.makedirs(ckpt_dir, exist_ok=True)
        os.makedirs(sample_dir, exist_ok=True)

    precision.set_activation_dtype(args.precision)
    torch.manual_seed(args.seed)               # identical replicas on every rank
    trainer = TS.build_trainer(args, "cpu", init_model)
    for v in trainer.values():
        if isinstance(v, torch.nn.Module):
            v.to(device)
    # Fuse FIRST, then resume: FusedAdamEMA.load_state_dict copies exp_avg_sq / step into its flat buffers and the module
    # load_state_dict copies into the flat parameter views, so the Adam state of the checkpoint survives (train.py:435-442).
    fuse_optimizers(trainer, args)
    if args.ckpt:
        # the reference resolves a bare name as experiments/<exp>/checkpoints/<ckpt>.pt (train.py:436-438); a path works too
        path = args.ckpt if os.path.isfile(args.ckpt) else f"{ckpt_dir}/{args.ckpt}.pt"
        print("load model:", path, flush=True)
        args.start_iter = checkpoint.load(path, trainer, map_location=device)
    if world > 1:
        # rank 0's weights, EMA copies and Adam state (a resumed rank 0 hands all three over): one broadcast per flat buffer of the
        # fused optimisers -- contiguous by construction, unlike the (o,ky,kx,i)-ordered 5-D modulated weights RCCL would reject
        broadcast_parameters([v for v in trainer.values() if isinstance(v, torch.nn.Module)],
                             optimizers=[trainer[k] for k in ("d_optim", "g_optim", "ex_optim")])
    reducer = GradReducer() if world > 1 else None
    random.seed(args.seed + 1000 + rank)       # crops and draws differ per rank, replicas do not
    torch.manual_seed(args.seed + 1000 + rank)

    dataset = D.set_dataset(args.dataset_type, args.dataset_path, args.image_size)
    sampler = D.data_sampler(dataset, shuffle=True, rank=rank, world=world, seed=args.seed)
    loader = D.DeviceLoader(dataset, args.batch_size, sampler, device=device, num_workers=args.num_workers,
                            seed=args.seed + rank, drop_last=True)
    short = len(loader) == 0
    if world > 1:
        # every rank must take the same exit: a rank that left alone would leave the others hanging in their first collective
        flag = torch.tensor([int(short)], device=device)
        dist.all_reduce(flag, op=dist.ReduceOp.MAX)
        if bool(flag.item()) and not short:
            dist.destroy_process_group()
            raise SystemExit(f"another rank's dataset shard holds fewer than --batch_size {args.batch_size} images; stopping with it")
    if short:
        if world > 1:
            dist.destroy_process_group()
        raise SystemExit(f"dataset shard of rank {rank} has {len(sampler)} images, fewer than --batch_size {args.batch_size}: "
                         "no full batch can be formed (lower --batch_size or add images)")
    if rank == 0:
        print(f"Data Loaded: {len(dataset)} images, {len(loader)} batches of {args.batch_size} per rank, {world} rank(s)", flush=True)

    batches = D.sample_data(loader)
    start_time = time.time()
    epoch_len = max(len(loader), 1)
    for idx in range(1, args.num_iters - args.start_iter + 1):
        iter_idx = idx + args.start_iter
        if (idx - 1) % epoch_len == 0:
            sampler.set_epoch((idx - 1) // epoch_len)
        X = next(batches)
        losses = TS.train_iteration(trainer, args, X, iter_idx, reducer=reducer)

        if iter_idx % args.log_every == 0 and rank == 0:               # train.py:223-247
            v = {k: float(t) for k, t in losses.items() if t.numel() == 1}
            used = time.time() - start_time
            rest = used / idx * (args.num_iters - iter_idx)
            line = (f"[{iter_idx:07d}/{args.num_iters:07}] Total: {v['Loss_total']:.4f}; "
                    f"G,rec: {v['G_rec_loss']:.4f}; G,texture: {v['G_texture_loss']:.4f}; G,real: {v['G_real_loss']:.4f}; "
                    f"E,dist: {v['E_dist_loss']:.4f}; E,stru: {v['E_stru_loss']:.4f}; Ex: {v['Ex_loss']:.4f} "
                    f"used time: {time_change(used)};rest time: {time_change(rest)}")
            print(line, flush=True)
            with open(f"{base_dir}/training_logs.txt", "a") as fp:
                fp.write(line + "\n")

        if iter_idx % args.show_every == 0 and rank == 0:              # train.py:249-303 (test block + image grid)
            with torch.no_grad():
                s = args.image_size // 16
                M = torch.randint(low=0, high=2, dtype=torch.float, size=(X.shape[0], args.N * s * s))
                T2 = torch.rand(X.shape[0], args.texture_channel, device=device) * 2 - 1
                use_x3 = iter_idx > args.num_iters * 0.8
                _, _, acc, l1, sample = TS.extraction_test(trainer, args, X, M, T2, use_x3, want_sample=True)
            line = (f"[Testing {iter_idx:07d}/{args.num_iters:07d}] sigma=1 delta=50% using synthesised image "
                    f"\\hatX_{3 if use_x3 else 2} ACC of Msg: {float(acc):.4f}; L1 loss of tensor: {float(l1):.4f}")
            print(line, flush=True)
            with open(f"{base_dir}/training_logs.txt", "a") as fp:
                fp.write(line + "\n")
            from ideas_amd.utils import save_image_grid                 # train.py:293-303: X / G(S1,T1) / G(S2,T1) / G(S2,T2), one row each
            save_image_grid(sample, f"{sample_dir}/{iter_idx:07d}.png", nrow=int(args.batch_size), value_range=(-1, 1))
            print(f"Sample images are saved in experiments/{args.exp_name}/samples", flush=True)

        if (iter_idx % args.save_every == 0 or iter_idx == args.num_iters) and rank == 0:    # train.py:308-322
            checkpoint.save(f"{ckpt_dir}/{iter_idx}.pt", trainer, args, iter_idx)   # the reference's file name

    if world > 1:
        if dist.get_backend() == "nccl":
            dist.barrier(device_ids=[device.index])
        else:
            dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
