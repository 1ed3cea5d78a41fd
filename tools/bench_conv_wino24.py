#!/usr/bin/env python3
"""Winograd F(2x4,3x3) (rpe_conv_wino24) vs F(2x2,3x3) (rpe_conv_wino) per layer: the update block's 3x3 shapes at batch 32 (64 x 80)
and the encoders' stride-1 shapes, with each kernel's max |error| against the f64 convolution on the first shape.
    python tools/bench_conv_wino24.py"""
import os, sys
import torch
import torch.nn.functional as F
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rpe_amd  # noqa: F401
from rpe_amd import ops


def t(fn, reps=20):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    a = torch.cuda.Event(enable_timing=True); b = torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps): fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3


dev = torch.device('cuda:0'); torch.manual_seed(0)
with torch.no_grad():
    for name, n, ci, co, h, w in (('convc2', 32, 256, 192, 64, 80), ('convf2', 32, 128, 64, 64, 80), ('conv', 32, 256, 126, 64, 80),
                                  ('fh1', 32, 128, 256, 64, 80), ('mask', 16, 128, 256, 64, 80), ('enc1/2', 32, 64, 64, 256, 320),
                                  ('enc1/4', 32, 96, 96, 128, 160), ('enc1/8', 32, 128, 128, 64, 80), ('convc2 b1', 1, 256, 192, 64, 80)):
        x = torch.randn(n, ci, h, w, device=dev); wt = torch.randn(co, ci, 3, 3, device=dev) * 0.05; bias = torch.randn(co, device=dev)
        o1 = torch.empty(n, co, h, w, device=dev); o2 = torch.empty_like(o1)
        p22, p24 = ops.PackedWino(wt, bias), ops.PackedWino24(wt, bias)
        t22 = t(lambda: ops.conv_wino(x, p22, ops.CONV_RELU, o1))
        t24 = t(lambda: ops.conv_wino(x, p24, ops.CONV_RELU, o2))
        line = '%-9s b%-2d %3d->%3d %3dx%3d   F(2x2) %8.1f us   F(2x4) %8.1f us   ratio %.3f' % (name, n, ci, co, h, w, t22, t24, t24 / t22)
        if name == 'convc2':
            xs = x[:2]
            ref = F.conv2d(xs.double(), wt.double(), bias.double(), padding=1).clamp_min(0)
            e22 = (ops.conv_wino(xs, p22, ops.CONV_RELU, o1[:2].clone()).double() - ref).abs().max().item()
            e24 = (ops.conv_wino(xs, p24, ops.CONV_RELU, o2[:2].clone()).double() - ref).abs().max().item()
            line += '   max|err| vs f64: F(2x2) %.2e  F(2x4) %.2e' % (e22, e24)
        print(line, flush=True)
