"""CPU: into which pieces raft_grad cuts a stride-1 weight gradient, ``conv_bwd_weight`` and ``sum_groups`` replaced by fakes that log their
calls -- no GPU, no library.  The conv_bwd_weight fake records the images it was handed (every image's x holds its batch index) and the
rows of the map on which dy is non-zero (dy is 1 everywhere, so a band is the rows that are left); it returns the sum of the dy it was
given in every element, so the pieces' f64 sum must come out as the whole map's b cout h w whichever way the map was cut.  Checked, for
each of the three policies (an update step without and with a gradient per iteration, an encoder's stride-1 layer without and with one)
at the sizes where the policy changes its mind: the number of launches, the images and rows of each piece, the number of sum_groups
calls and their group count."""
import pytest
import torch


@pytest.fixture()
def fakes(rpe, monkeypatch):
    from rpe_amd import raft_grad
    log = []

    def conv_bwd_weight(x, dy, kernel, scale=1.0, bias=True):
        assert scale == 1.0 and x.shape[0] == dy.shape[0] and x.shape[2:] == dy.shape[2:]
        live = [r for r in range(dy.shape[2]) if bool(dy[:, :, r].any())]
        assert live == list(range(live[0], live[-1] + 1)) and bool((dy[:, :, live] == 1).all())          # whole rows, one run of them
        log.append(('wgrad', tuple(int(v) for v in x[:, 0, 0, 0]), (live[0], live[-1] + 1)))
        total = float(dy.sum())
        return torch.full((dy.shape[1], x.shape[1], *kernel), total), (torch.full((dy.shape[1],), total) if bias else None)

    def sum_groups(parts, bias=None, relu=False, out=None):
        assert bias is None and not relu and out is None and parts.dim() == 5 and parts.is_contiguous() and parts.shape[0] > 1
        log.append(('sum', parts.shape[0]))
        return parts.double().sum(0).float()
    monkeypatch.setattr(raft_grad, 'conv_bwd_weight', conv_bwd_weight)
    monkeypatch.setattr(raft_grad, 'sum_groups', sum_groups)
    return raft_grad, log


def _update(raft_grad, x, dy, kernel, bands, bias=True):
    """An update step's weight gradient as update_step_backward(wgrad_bands=bands) forms it."""
    return raft_grad._split_bwd_weight(x, dy, kernel, bias, **(raft_grad._UPDATE_BANDS if bands else {}))


def _encoder(raft_grad, x, dy, kernel, bands, bias=True):
    """An encoder's stride-1 layer's as encoder_backward(wgrad_bands=bands) forms it."""
    return raft_grad._split_bwd_weight(x, dy, kernel, bias, **(raft_grad._ENCODER_BANDS if bands else raft_grad._ENCODER))


def _run(fakes, which, b, hh, ww, bands, bias=True, kernel=(3, 3), cin=3, cout=2):
    """-> (the launches [(images, (row lo, row hi))], the sum_groups calls' group counts); the result checked against the whole map's."""
    raft_grad, log = fakes
    del log[:]
    x = torch.arange(b, dtype=torch.float32).view(b, 1, 1, 1).expand(b, cin, hh, ww).contiguous()
    dy = torch.ones(b, cout, hh, ww)
    dw, db = which(raft_grad, x, dy, kernel, bands, bias)
    assert tuple(dw.shape) == (cout, cin, *kernel) and bool((dw == b * cout * hh * ww).all())
    assert (db is None) == (not bias) and (db is None or (tuple(db.shape) == (cout,) and bool((db == b * cout * hh * ww).all())))
    assert bool((dy == 1).all())                                        # the caller's gradient is not written
    launches = [e[1:] for e in log if e[0] == 'wgrad']
    assert log[:len(launches)] == [('wgrad',) + e for e in launches]    # every piece's launch, then the sums
    return launches, [e[1] for e in log[len(launches):]]


def _bands(images, hh, rows):
    return [(images, (lo, min(hh, lo + rows))) for lo in range(0, hh, rows)]


def test_update_step_without_a_gradient_per_iteration_is_one_launch(fakes):
    for b, hh, ww in ((1, 8, 8), (1, 16, 16), (2, 16, 16), (1, 32, 33)):
        assert _run(fakes, _update, b, hh, ww, False) == ([(tuple(range(b)), (0, hh))], [])


def test_update_step_bands(fakes):
    assert _run(fakes, _update, 1, 8, 8, True) == ([((0,), (0, 8))], [])               # one band of 64 pixels covers the map
    assert _run(fakes, _update, 1, 16, 16, True) == (_bands((0,), 16, 4), [4, 4])      # bands of 4 rows; the weight's sum and the bias's
    assert _run(fakes, _update, 1, 16, 16, True, kernel=(1, 5)) == (_bands((0,), 16, 4), [4, 4])
    assert _run(fakes, _update, 2, 16, 16, True) == (_bands((0, 1), 16, 2), [8, 8])    # a band's 64 pixels count both images' rows
    assert _run(fakes, _update, 1, 32, 32, True) == (_bands((0,), 32, 2), [16, 16])    # 1024 pixels: still in bands
    assert _run(fakes, _update, 1, 32, 33, True) == ([((0,), (0, 32))], [])            # 1056 > 1024: the kernel chunks the map itself
    assert _run(fakes, _update, 1, 3, 100, True) == (_bands((0,), 3, 1), [3, 3])       # a row longer than a band: one row each


def test_encoder_layer_without_bands(fakes):
    assert _run(fakes, _encoder, 1, 16, 16, False) == ([((0,), (0, 16))], [])
    assert _run(fakes, _encoder, 2, 16, 16, False) == ([((0,), (0, 16)), ((1,), (0, 16))], [2, 2])      # one image each
    assert _run(fakes, _encoder, 2, 16, 16, False, bias=False) == ([((0,), (0, 16)), ((1,), (0, 16))], [2])
    assert _run(fakes, _encoder, 4, 16, 16, False, kernel=(1, 1)) == ([((i,), (0, 16)) for i in range(4)], [4, 4])      # 1024 pixels: still per image
    assert _run(fakes, _encoder, 2, 24, 24, False) == ([((0, 1), (0, 24))], [])        # 1152 > 1024: one launch


def test_encoder_layer_with_bands(fakes):
    assert _run(fakes, _encoder, 1, 16, 16, True) == ([((0,), (0, 16))], [])           # at most 1024 pixels: as without bands
    assert _run(fakes, _encoder, 2, 16, 16, True) == ([((0,), (0, 16)), ((1,), (0, 16))], [2, 2])
    assert _run(fakes, _encoder, 1, 32, 32, True) == ([((0,), (0, 32))], [])           # 1024 pixels, 8 rows to a band: still one launch
    assert _run(fakes, _encoder, 2, 24, 24, True) == (_bands((0, 1), 24, 5), [5, 5])   # 256 // (2 x 24) = 5 rows: 5 launches
    assert _run(fakes, _encoder, 2, 24, 24, True, bias=False) == (_bands((0, 1), 24, 5), [5])
    assert _run(fakes, _encoder, 1, 64, 64, True) == (_bands((0,), 64, 4), [16, 16])   # 4096 pixels: still in bands
    assert _run(fakes, _encoder, 1, 64, 65, True) == ([((0,), (0, 64))], [])           # 4160 > 4096: one launch
    assert _run(fakes, _encoder, 1, 4, 300, True) == (_bands((0,), 4, 1), [4, 4])      # a row longer than a band: one row each
