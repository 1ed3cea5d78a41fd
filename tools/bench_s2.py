#!/usr/bin/env python3
"""The encoders' stride-2 layers at bench geometry (fnet: 48 images, moments; cnet: 16 images, folded batch norm + ReLU): 3x3 stride 2 and
the 1x1 stride-2 shortcut.  The 64 -> 96 3x3 layers are timed on both tile classes, alternated in one process: rpe_conv_fused's 128-row
tiles and rpe_conv_fused_m96's 96-row tiles (csrc/conv_s2.hip)."""
import os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rpe_amd
from rpe_amd import ops
from bench_kernels import timeit
dev = torch.device('cuda:0'); torch.manual_seed(0)
for nb in (48, 16):
    for name, cin, cout, k, h, w in (('layer2.conv1 3x3 s2', 64, 96, 3, 256, 320), ('layer2.shortcut 1x1 s2', 64, 96, 1, 256, 320),
                                     ('layer3.conv1 3x3 s2', 96, 128, 3, 128, 160), ('layer3.shortcut 1x1 s2', 96, 128, 1, 128, 160)):
        x = torch.randn(nb, cin, h, w, device=dev); wt = torch.randn(cout, cin, k, k, device=dev) * 0.05; bias = torch.randn(cout, device=dev)
        out = torch.empty(nb, cout, h // 2, w // 2, device=dev)
        pc = ops.PackedConv(wt, bias)
        st = ops.conv_stats_buffer(nb, cout, h, w, dev, stride=2) if nb == 48 else None
        kw = dict(stats=st) if nb == 48 else dict(scale=bias.abs() + 0.5, bias=bias)
        mode = ops.CONV_LINEAR if nb == 48 else ops.CONV_RELU
        fl = 2.0 * nb * (h // 2) * (w // 2) * cin * cout * k * k
        gb = (x.numel() * (0.5 if k == 1 else 1.0) + out.numel()) * 4 / 1e9
        entries = ('rpe_conv_fused', 'rpe_conv_fused_m96') if (k, cout) == (3, 96) else ('rpe_conv_fused',)
        for rnd in range(3 if len(entries) > 1 else 1):                                     # alternated rounds
            for entry in entries:
                med, mn = timeit(lambda: ops.conv_fused(x, pc, mode, out, stride=2, entry=entry, **kw), 20)
                print(f'{name:24s} x{nb} {entry[4:]:15s}: {med:8.1f} us (min {mn:.1f})  {fl / med / 1e6:6.1f} TFLOP/s  {gb / med * 1e6 / 1e3:5.2f} TB/s of input rows + output')
