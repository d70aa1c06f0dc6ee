"""One StyleGAN2 discriminator step on ``ideas_amd.model.Discriminator`` (stylegan2/train.py's D phase with its R1 branch, f32):
logistic loss on a real and a fake batch -> backward, then the R1 penalty on the real batch -> backward.  Prints the wall time of
a step; run it under ``rocprofv3 --kernel-trace --stats`` for the per-kernel times (every step, warm-up included, launches the
same kernels: divide the totals by STEPS + WARMUP).   env: SIZE (256), B (32), STEPS (3), WARMUP (2)"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from ideas_amd.model import Discriminator
from ideas_amd.utils import d_r1_loss

SIZE, B = int(os.environ.get("SIZE", 256)), int(os.environ.get("B", 32))
STEPS, WARMUP = int(os.environ.get("STEPS", 3)), int(os.environ.get("WARMUP", 2))
torch.manual_seed(0)
net = Discriminator(SIZE).cuda()
real = (torch.rand(B, 3, SIZE, SIZE, device="cuda") * 2 - 1).contiguous(memory_format=torch.channels_last)
fake = (torch.rand(B, 3, SIZE, SIZE, device="cuda") * 2 - 1).contiguous(memory_format=torch.channels_last)


def step():
    net.zero_grad(set_to_none=True)
    loss = F.softplus(-net(real)).mean() + F.softplus(net(fake)).mean()
    loss.backward()
    x = real.detach().requires_grad_(True)
    pred = net(x)
    (10 / 2 * d_r1_loss(pred, x) * 16 + 0 * pred[0]).sum().backward()


for _ in range(WARMUP):
    step()
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(STEPS):
    step()
torch.cuda.synchronize()
print(f"Discriminator({SIZE}) B={B} D step (forward, backward, R1): {(time.perf_counter() - t0) / STEPS * 1e3:.1f} ms wall, "
      f"{STEPS} steps after {WARMUP} warm-up")
