"""GPU: the launches of a RAFT pass, pinned.  tests/golden/raft_launch_traces.json holds, for ten small passes (2 iterations, batch 1) that
between them take every route raft.py chooses between, the entry points the pass calls in order -- dispatched launch by launch from
Python, and on the default route: the replayed pass's calls and the update loop's launch list with the stream of every op.  A change to
raft.py's host side that is meant to leave the launches alone must reproduce them exactly.

``python tests/test_gpu_raft_launch_trace.py [path]`` rewrites the fixture (or writes ``path``) from the raft.py it is run against: do
that only for a change that is meant to move a launch, and say so."""
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'raft_launch_traces.json')
ITERS = 2
# case -> (config keys, (H, W), forward keywords; 'warm' stands for flow_init = zeros)
# 128 x 160 is the smallest size of this suite's RAFT tests (tests/test_conv_f16_host.py says why); 136 x 152 is the nearest size with an
# odd map (17 x 19, w8 % 4 != 0: the generic route) that padded_size changes in both directions and whose fourth correlation level still
# has two rows (a 15-row map's has one, which rpe_corr_pyramid_bytes refuses)
CASES = {'default': ({}, (128, 160), {}),
         'generic': ({}, (136, 152), {}),
         'pad_maps': (dict(pad_maps=True), (136, 152), {}),
         'pad_both': (dict(pad_maps=True, pad_encoders=True), (136, 152), {}),
         'alt': (dict(alternate_corr=True), (128, 160), {}),
         'alt16': (dict(alternate_corr=True, alt_corr_fp16=True), (128, 160), {}),
         'f16': (dict(update_fp16=True), (128, 160), {}),
         'mp_f16': (dict(mixed_precision=True, update_fp16=True), (128, 160), {}),
         'warm': ({}, (128, 160), dict(warm=True, ret_lowres=True)),
         'all_flows': ({}, (128, 160), dict(all_flows=True))}
EVENT_OPS = {32: 'event_record', 33: 'stream_wait'}                          # (_lib.OP_EVENT_RECORD / OP_STREAM_WAIT: no argument struct)


def make_case(name, weights=None):
    """(model on the GPU, forward's arguments) of a case; every case has the same synthetic weights."""
    from rpe_amd import raft, synth
    cfg, (H, W), kw = CASES[name]
    net = raft.RAFT(synth.model_config(H, W, iters=ITERS, **cfg)).eval()
    if weights is None:
        synth.init_synthetic_weights(net)
    else:
        net.load_state_dict(weights)
    net = net.cuda()
    fr = synth.stereo_frames(7, 1, H, W)
    kw = dict(kw)
    if kw.pop('warm', False):
        kw['flow_init'] = torch.zeros(1, 2, H // 8, W // 8, device='cuda')
    return net, (fr['image1l'].cuda(), fr['image2l'].cuda()), dict(kw, iters=ITERS)


def _counted(net, images, kw, warm):
    from rpe_amd import _lib
    with torch.no_grad():
        for _ in range(warm):                                                 # (the first pass makes the packings, the second is recorded)
            net(*images, **kw)
        with _lib.CountingLib() as count:
            out = net(*images, **kw)
    torch.cuda.synchronize()
    return count.names, out


def trace(name, weights=None):
    """The trace of one case: {'direct': the calls of a pass dispatched from Python, and the entry point behind every prepared launcher of
    the update loop (those call the library themselves), 'lists': the calls of a replayed pass on the default route, and the update
    loop's launch list as (entry point, stream index)}; and the outputs of the default route's pass."""
    from rpe_amd import _lib, raft
    entry = lambda kind: EVENT_OPS.get(kind) or _lib.ALL_LIST_OPS[kind][0]
    net, images, kw = make_case(name, weights)
    old = raft.FRAME_OPLISTS, raft.LOOP_OPLIST
    try:
        raft.FRAME_OPLISTS = raft.LOOP_OPLIST = False
        names, _ = _counted(net, images, kw, warm=1)
        prepared = []
        for ws in net._ws.values():
            if '_launchers' in ws:
                L = ws['_launchers'][1]
                prepared = [[n, entry(getattr(L, n).op[0])] for n in ('c1', 'c2', 'f1', 'f2', 'cv')] + [['gru', entry(g.op[0])] for g in L.gru]
        direct = dict(names=list(names), prepared=prepared)
        raft.FRAME_OPLISTS = raft.LOOP_OPLIST = True
        net, images, kw = make_case(name, weights)                            # a fresh model: nothing of the other route is cached
        names, out = _counted(net, images, kw, warm=2)
        loop = []
        for ws in net._ws.values():
            if '_program' in ws:
                loop = [[entry(kind), stream] for kind, stream, _ in ws['_program'][1][0]._items]
        lists = dict(names=list(names), loop=loop)
    finally:
        raft.FRAME_OPLISTS, raft.LOOP_OPLIST = old
    return dict(direct=direct, lists=lists), out


@pytest.fixture(scope='module')
def weights(rpe):
    from rpe_amd import raft, synth
    return synth.init_synthetic_weights(raft.RAFT(synth.model_config(128, 160, iters=ITERS))).state_dict()


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(CASES))
def test_launches_are_the_recorded_ones(rpe, weights, name):
    want = json.load(open(FIXTURE))[name]
    got, out = trace(name, weights)
    for route in ('direct', 'lists'):
        for part in want[route]:
            assert got[route][part] == want[route][part], (name, route, part)
    assert want['direct']['names'] and ('rpe_run_ops' in want['lists']['names'] and want['lists']['loop'] or name == 'generic')
    H, W = CASES[name][1]
    assert out[0][-1].shape == (1, 2, H, W) and out[1].shape == (1, 128, H // 8, W // 8) and bool(torch.isfinite(out[0][-1]).all())


if __name__ == '__main__':
    sys.path.insert(0, ROOT)
    import rpe_amd  # noqa: F401
    path = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    with open(path, 'w') as f:
        json.dump({name: trace(name)[0] for name in CASES}, f, indent=0, sort_keys=True)
        f.write('\n')
    print('wrote', path)
