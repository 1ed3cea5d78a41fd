"""GPU: one-launch (persistent) pose solves running at the same time as each other, as heavy memory traffic and as the RAFT encoders.

In a persistent solve a row's workgroups hand partial sums and poses to each other through memory, on any XCD (csrc/pose.hip,
k_pose_reduce's tail; the instruction order that makes the handoff safe is checked on the CPU by test_pose_publish_isa.py).  On an idle
device the window in which a stale partial row or pose line could be read is tiny; here four solves share the chip with each other and
with a stream copying gigabytes through HBM and the L2s, round after round.  Every output -- T, vec7, log6, info -- must equal, bit for
bit, the same case solved alone with one launch per evaluation (RPE_SOLVE_LAUNCH_PER_EVALUATION).

Co-residency is part of the test: a persistent solve's workgroups wait for their row's tail without yielding their slot, so concurrent
solves whose grids together exceed the device can starve each other (include/rpe.h, rpe_solve_opts).  The combined grid of the
concurrent solves is kept at or below HALF the device's resident capacity, asserted before anything is launched."""
import pytest
import torch

from oracle import synth

SOLVER_LBFGS, SOLVER_GN = 0, 1
RED_THREADS = 256
ROUNDS = 20
COPY_BYTES = 256 << 20          # x 8 copies per round = 2 GiB through HBM beside the solves


def pose_nblk(n, h, w, hess):
    """csrc/pose.hip pose_nblk: workgroups per row of the default partition (one resident round chip-wide)."""
    quads = (h * w + 3) // 4
    per_row = (quads + RED_THREADS * 2 - 1) // (RED_THREADS * 2)
    want = ((512 if hess else 768) + n - 1) // n
    nblk = max(1, min(per_row, want))
    return min(nblk, (quads + RED_THREADS - 1) // RED_THREADS, 2048)


def resident_capacity(hess):
    """Workgroups of k_pose_reduce the device holds at once: __launch_bounds__(256, 3), (256, 2) with the Hessian."""
    return torch.cuda.get_device_properties(0).multi_processor_count * (2 if hess else 3)


def cases(mode):
    """(args, iters) of the four concurrent solves: a full frame, a row that is optimal at the start (mask1 all false), a NaN row, and a
    map whose width is not a multiple of 4 (the scalar-load kernel)."""
    hess = mode == SOLVER_GN
    full = synth.solver_args(synth.solver_case(41, 1, 320, 512) if hess else synth.solver_case(41, 1, 512, 640))
    masked = [t.clone() for t in synth.solver_args(synth.solver_case(42, 2, 256, 320))]
    masked[5][1] = False
    nan = [t.clone() for t in synth.solver_args(synth.solver_case(43, 5, 64, 96))]
    nan[0][3, 0, 7, 11] = float('nan')
    scalar = synth.solver_args(synth.solver_case(44, 3, 37, 53))
    return [(full, 20), (masked, 8), (nan, 8), (scalar, 8)]


def grid(args, mode):
    n, _, h, w = args[0].shape
    return n * pose_nblk(n, h, w, mode == SOLVER_GN)


def same(x, y):
    """Bit-equal, with NaN where NaN is (test_gpu_pose.py's comparison)."""
    return torch.equal(x, y) or (torch.isnan(x) == torch.isnan(y)).all() and torch.equal(torch.nan_to_num(x), torch.nan_to_num(y))


def alone(ops, args, iters, mode):
    """The reference: solved by itself on an idle device, one launch per evaluation."""
    torch.cuda.synchronize()
    out = [t.cpu() for t in ops.pose_solve(*args, iters=iters, mode=mode, persistent=False)]
    torch.cuda.synchronize()
    return out


def test_restated_partition_matches_the_library(rpe):
    """pose_nblk above is the library's: rpe_pose_workspace_bytes(1, h, w) holds 32 doubles per workgroup of the single-row partition."""
    L = rpe.lib()
    base = L.rpe_pose_workspace_bytes(1, 1, 1)                          # one workgroup
    for h, w in ((512, 640), (320, 512), (256, 320), (64, 96), (37, 53), (1, 1), (700, 900)):
        assert (L.rpe_pose_workspace_bytes(1, h, w) - base) // 256 + 1 == pose_nblk(1, h, w, False), (h, w)


@pytest.mark.gpu
@pytest.mark.parametrize('mode', [SOLVER_LBFGS, SOLVER_GN])
def test_concurrent_one_launch_solves_under_memory_traffic(rpe, mode):
    from rpe_amd import ops
    hess = mode == SOLVER_GN
    work = [([t.cuda() for t in a], k) for a, k in cases(mode)]
    total = sum(grid(a, mode) for a, _ in work)
    cap = resident_capacity(hess)
    assert total <= cap // 2, f'the concurrent grids ({total} workgroups) must stay within half the resident capacity ({cap})'
    ref = [alone(ops, a, k, mode) for a, k in work]

    cur = torch.cuda.current_stream()
    streams = [torch.cuda.Stream() for _ in work]
    copier = torch.cuda.Stream()
    src = torch.empty(COPY_BYTES, dtype=torch.uint8, device='cuda').random_()
    dst = torch.empty_like(src)
    for r in range(ROUNDS):
        copier.wait_stream(cur)
        with torch.cuda.stream(copier):
            for _ in range(4):
                dst.copy_(src)
                src.copy_(dst)
        outs = []
        for s, (a, k) in zip(streams, work):
            s.wait_stream(cur)
            with torch.cuda.stream(s):
                outs.append(ops.pose_solve(*a, iters=k, mode=mode, persistent=True))
        torch.cuda.synchronize()
        for i, (o, e) in enumerate(zip(outs, ref)):
            for name, x, y in zip(('T', 'vec7', 'log6', 'info'), o, e):
                assert same(x.cpu(), y), f'round {r}, solve {i}: {name} differs from the solve alone'


@pytest.mark.gpu
@pytest.mark.parametrize('mode', [SOLVER_LBFGS, SOLVER_GN])
def test_one_launch_solve_beside_the_raft_encoders(rpe, mode):
    """The product's overlap: RAFT's encoders (feature encoder, and the context encoder on RAFT's own side stream: 8 images) run on a
    side stream while a solve runs on the current stream -- the pose must be the one of the same solve alone."""
    from rpe_amd import ops, pose_net
    from rpe_amd import synth as rsynth
    h, w = 256, 320
    model = rsynth.init_synthetic_weights(pose_net.PoseNet(rsynth.model_config(h, w)), seed=5).eval().cuda()
    fr = rsynth.stereo_frames(6, 8, h, w)
    L, R = fr['image2l'].cuda(), fr['image2r'].cuda()
    (a, k) = cases(mode)[0]
    a = [t.cuda() for t in a]
    assert grid(a, mode) <= resident_capacity(mode == SOLVER_GN) // 2
    ref = alone(ops, a, k, mode)
    cur = torch.cuda.current_stream()
    side = torch.cuda.Stream()
    for r in range(5):
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            enc = model.flow.encode_both((L, R), L)
        out = ops.pose_solve(*a, iters=k, mode=mode, persistent=True)
        torch.cuda.synchronize()
        for name, x, y in zip(('T', 'vec7', 'log6', 'info'), out, ref):
            assert same(x.cpu(), y), f'round {r}: {name} differs from the solve alone'
        assert all(bool(torch.isfinite(t).all()) for t in enc)
        del enc
