"""GPU: the twelve small kernels of csrc/raft_ops.hip (GRU gates, bias/activation, instance norm and affine epilogues, the 3x3 -> 2 flow
head with its coords / flow bookkeeping, convex 8x up-sampling, plane and rectangle copies) at the launches their short tests in
tests/test_gpu_corr.py never make, against the float64 restatements of tests/raft_ops_ref.py (pinned on the CPU by
tests/test_raft_ops_ref_cpu.py).

Every comparison is ``raft_ops_ref.compare``: no element is left out; NaN must sit exactly where the reference has it, +-Inf likewise and
with the same sign, everything else is compared numerically.

What the cases are for:
  * flow head: the four-pixels-per-thread kernel at maps of one group per row, one and two rows, odd channel slices (the tail after the
    two-channel unrolled loop), empty wave slices and a partial last wave -- forced by a large batch, since ``launch_to2`` takes it only from
    256 workgroups on (the condition is recomputed and asserted here); the same items launched alone take the one-pixel kernel and must
    give the same bits; Inf / NaN / 1e30 markers at corners, row ends and around lane 0 and lane 63; misaligned bases;
  * element-wise kernels: a launch large enough for a second grid-stride trip (more than 2048 * 256 * VEC elements per item) in both vector
    classes, bases offset by one float, gate pre-activations from 0 to +-Inf;
  * instance norm: the 256- and 512-thread classes on both sides of 16384, planes of 1 and 3 elements, constant and large-mean planes;
  * up-sampling: maps of one cell, one row, one column, one block exactly and one cell more; logits of sigma 80, +-1e4 spikes, -Inf, +Inf,
    nine equal logits; flow with 1e6, Inf and NaN pixels; one pitched call.

Bars that are not fixed numbers are 4x the error of torch's own float32 operator against the same float64 truth on the same input; both
errors are printed.  Measured values are in the docstrings of the tests that use them."""
import functools

import pytest
import torch
import torch.nn.functional as F

import raft_ops_ref as ref
from oracle import raft as oraft

pytestmark = pytest.mark.gpu

DEV = 'cuda'
NAN, INF = float('nan'), float('inf')


def shifted(t):
    """A contiguous GPU copy of ``t`` whose storage starts one float into an allocation: its base is not 16-byte aligned."""
    buf = torch.empty(t.numel() + 1, dtype=torch.float32, device=DEV)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def same_bits(a, b):
    """torch.equal that lets NaN equal NaN."""
    a, b = a.cpu(), b.cpu()
    return a.shape == b.shape and torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0))


# ====================================================================================================================== flow head
TO_WAVES = 8                                              # TO1_WAVES = TO2_WAVES of raft_ops.hip: channel slices per workgroup
WSCALE = 0.05                                             # the weight scale of test_flow_head_kernels_agree_bitwise: its 2e-4 bar carries over
FLOW_BAR = 2e-4


def takes_x4(b, h, w):
    """launch_to2's choice for 16-byte-aligned tensors: the four-pixel kernel needs w % 4 == 0 and at least 256 workgroups."""
    return w % 4 == 0 and -(-(h * w // 4) // 64) * b >= 256


# (b, C, h, w, takes the four-pixel kernel).  The row (128, 20, 9, 28) is below the launch threshold (one workgroup per item, 128 in all) and so
# checks the one-pixel kernel only; (256, 20, 9, 28) is the same map in a batch that does reach the four-pixel kernel.
X4_CASES = [(256, 37, 3, 4, True),                        # cq = 5: odd slice, the tail after the unrolled loop; one group per row
            (256, 5, 1, 8, True),                         # C < 8: empty wave slices; one row
            (256, 9, 2, 12, True),                        # two rows: top and bottom both clamped
            (256, 24, 16, 16, True),                      # cq = 3; exactly one full wave per item
            (128, 20, 9, 28, False),
            (256, 20, 9, 28, True),                       # 63 groups: the last lane idle, edge lane 63 outside the map
            (86, 256, 11, 68, True)]                      # three workgroups per item, the last one partial


@functools.lru_cache(maxsize=2)
def flow_case(b, c, h, w):
    g = torch.Generator().manual_seed(1000 * c + 10 * h + w)
    x = torch.randn(b, c, h, w, generator=g)
    wt, bias = torch.randn(2, c, 3, 3, generator=g) * WSCALE, torch.randn(2, generator=g)
    add = torch.randn(b, 2, h, w, generator=g) * 10
    plain = ref.conv3x3_to2(x, wt, bias)
    return x, wt, bias, add, plain


@pytest.mark.parametrize('b,c,h,w,x4', X4_CASES)
def test_flow_head_four_pixel_kernel_at_small_maps(rpe, b, c, h, w, x4):
    """Against float64 at the 2e-4 bar of test_flow_head_kernels_agree_bitwise, and items 0, 1 and b - 1 launched alone (one-pixel kernel)
    bit-equal to their rows of the batched launch."""
    from rpe_amd import ops
    assert takes_x4(b, h, w) == x4 and not takes_x4(1, h, w)          # else both launches below would take the same kernel
    x, wt, bias, add, plain = flow_case(b, c, h, w)
    xd, wd, bd, ad = x.to(DEV), wt.to(DEV), bias.to(DEV), add.to(DEV)
    big, big_add = ops.conv3x3_to2(xd, wd, bd), ops.conv3x3_to2(xd, wd, bd, add=ad)
    e0 = ref.compare(big, plain, FLOW_BAR, 'batched')
    e1 = ref.compare(big_add, plain + add.double(), FLOW_BAR, 'batched + add')
    print(f'flow head {(b, c, h, w)}: max error {e0:.3e}, with add {e1:.3e} (bar {FLOW_BAR:.0e})')
    for i in (0, 1, b - 1):
        assert torch.equal(ops.conv3x3_to2(xd[i:i + 1].contiguous(), wd, bd), big[i:i + 1]), i
        assert torch.equal(ops.conv3x3_to2(xd[i:i + 1].contiguous(), wd, bd, add=ad[i:i + 1].contiguous()), big_add[i:i + 1]), i


# Markers: a 44 x 12 map has three groups of four per row, so group 64 (lane 0 of the second workgroup) is row 21, x0 = 4 and group 127 (its
# lane 63) is row 42, x0 = 4: both have a left and a right neighbour group.  C = 11: cq = 2, wave 5 holds one channel (the tail loop), waves
# 6 and 7 none.
MB, MC, MH, MW = 256, 11, 44, 12
ROW_Y = 10                                                # 1e30 at the last pixel of this row and at the first pixel of the next


def marker_case():
    g = torch.Generator().manual_seed(77)
    x = torch.randn(MB, MC, MH, MW, generator=g)
    wt, bias = torch.randn(2, MC, 3, 3, generator=g) * WSCALE, torch.randn(2, generator=g)
    add = torch.randn(MB, 2, MH, MW, generator=g) * 10
    clean = x[0].clone()
    for (y, xx) in ((0, 0), (0, MW - 1), (MH - 1, 0), (MH - 1, MW - 1)):
        x[0, 1, y, xx] = INF
    x[0, 2, 30, 6] = NAN
    x[0, 3, ROW_Y, MW - 1] = 1e30
    x[0, 4, ROW_Y + 1, 0] = 1e30
    x[0, 5, 21, 3], x[0, 6, 21, 8] = 3e4, -5e4            # x0 - 1 and x0 + 4 of the group on lane 0
    x[0, 7, 42, 3], x[0, 8, 42, 8] = -3e4, 5e4            # ... and of the group on lane 63
    return x, wt, bias, add, clean


def marker_bar(x, wt, bias, add):
    """2e-4 where the existing bar can hold, and the forward error bound of the kernel's own summation where a 1e30 or 3e4 marker makes the
    terms large: n * 2^-24 * sum |term| with n = 9 * cq + 10 roundings on the longest chain (9 fused multiply-adds per channel of a slice,
    7 additions across the slices, bias, add, and one to spare)."""
    n = 9 * -(-x.shape[1] // TO_WAVES) + 10
    mag = ref.conv3x3_to2(torch.nan_to_num(x, nan=0.0, posinf=0.0, neginf=0.0).abs(), wt.abs(), bias.abs(), None if add is None else add.abs())
    return torch.clamp(n * 2.0 ** -24 * mag, min=FLOW_BAR)


def check_marker_output(out, want, bar, what):
    ref.compare(out, want, bar, what)
    o = out.cpu()
    inf_at, nan_at = torch.zeros(MH, MW, dtype=torch.bool), torch.zeros(MH, MW, dtype=torch.bool)
    inf_at[:2, :2] = inf_at[:2, -2:] = inf_at[-2:, :2] = inf_at[-2:, -2:] = True        # a corner Inf: its in-map 2x2 neighbourhood
    nan_at[29:32, 5:8] = True
    for ch in range(2):
        assert torch.equal(torch.isinf(o[0, ch]), inf_at) and torch.equal(torch.isnan(o[0, ch]), nan_at), (what, ch)
    assert bool(torch.isfinite(o[1:]).all()), what                      # (empty for a launch of item 0 alone)


@pytest.mark.parametrize('with_add', (False, True))
def test_flow_head_nonfinite_and_row_end_markers(rpe, with_add):
    """Inf at the four corners, a NaN inside, 1e30 at a row's last pixel and the next row's first, markers left and right of the groups on lane 0
    and lane 63: both kernels (item 0 alone, and in the batch of 256) against float64, the non-finite set exactly the corners' 2x2 and the NaN's
    3x3, and the first column of the rows around ROW_Y + 1 the same bits with and without the marker at the end of row ROW_Y."""
    from rpe_amd import ops
    assert takes_x4(MB, MH, MW) and not takes_x4(1, MH, MW)
    x, wt, bias, add, clean = marker_case()
    a = add if with_add else None
    want, bar = ref.conv3x3_to2(x, wt, bias, a), marker_bar(x, wt, bias, a)
    xd, wd, bd = x.to(DEV), wt.to(DEV), bias.to(DEV)
    ad = add.to(DEV) if with_add else None
    big = ops.conv3x3_to2(xd, wd, bd, add=ad)
    alone = ops.conv3x3_to2(xd[:1].contiguous(), wd, bd, add=None if ad is None else ad[:1].contiguous())
    check_marker_output(big, want, bar, 'batched')
    check_marker_output(alone, want[:1], bar[:1], 'alone')
    assert same_bits(alone, big[:1])
    # the last pixel of row ROW_Y must not reach the first group of the rows below: take that marker out and look at column 0
    x2 = x.clone()
    x2[0, 3, ROW_Y, MW - 1] = clean[3, ROW_Y, MW - 1]
    x2d = x2.to(DEV)
    for got, other in ((big, ops.conv3x3_to2(x2d, wd, bd, add=ad)),
                       (alone, ops.conv3x3_to2(x2d[:1].contiguous(), wd, bd, add=None if ad is None else ad[:1].contiguous()))):
        assert torch.equal(got[0, :, ROW_Y - 1:ROW_Y + 4, 0], other[0, :, ROW_Y - 1:ROW_Y + 4, 0])
        assert not torch.equal(got[0, :, ROW_Y, MW - 2:], other[0, :, ROW_Y, MW - 2:])          # (the marker does reach its own neighbours)


def test_flow_head_markers_through_flow_update(rpe):
    """The same markers through rpe_conv3x3_to2_flow with all three extra destinations: coords_out against float64, and flow_out, dst1, dst2
    bit-equal to coords_out - grid in every cell, the non-finite ones included; nothing outside the two-channel slices is written."""
    from rpe_amd import ops
    x, wt, bias, add, _ = marker_case()
    grid = oraft.coords_grid(MB, MH, MW)
    coords = (grid + add)
    want, _ = ref.flow_update(x, wt, bias, coords)
    bar = marker_bar(x, wt, bias, coords)
    xd, wd, bd, cd, gd = x.to(DEV), wt.to(DEV), bias.to(DEV), coords.to(DEV), grid.to(DEV)
    for rows in (slice(0, MB), slice(0, 1)):                              # four-pixel kernel, one-pixel kernel
        n = rows.stop
        hx, rhx = torch.full((n, 256, MH, MW), -7.0, device=DEV), torch.full((n, 256, MH, MW), -7.0, device=DEV)
        flow, out = torch.full((n, 2, MH, MW), -7.0, device=DEV), torch.full((n, 2, MH, MW), -7.0, device=DEV)
        got = ops.flow_update(xd[rows].contiguous(), wd, bd, cd[rows].contiguous(), out, flow_out=flow, dst1=hx[:, 254:], dst2=rhx[:, 254:])
        assert got is out
        check_marker_output(out, want[rows], bar[rows], f'flow_update x{n}')
        fl = out - gd[rows]
        for name, dst in (('flow_out', flow), ('dst1', hx[:, 254:]), ('dst2', rhx[:, 254:])):
            assert same_bits(dst, fl), (n, name)
        assert bool((hx[:, :254] == -7.0).all()) and bool((rhx[:, :254] == -7.0).all())


def test_flow_head_misaligned_bases_take_the_one_pixel_kernel(rpe):
    """x, add, out or a destination slice whose base is one float into an allocation: not fit for the four-pixel kernel's float4 accesses, so
    the launch falls back to the one-pixel kernel, which gives the same bits."""
    from rpe_amd import ops
    b, c, h, w = 256, 9, 2, 12
    assert takes_x4(b, h, w)
    x, wt, bias, add, _ = flow_case(b, c, h, w)
    xd, wd, bd, ad = x.to(DEV), wt.to(DEV), bias.to(DEV), add.to(DEV)
    want = ops.conv3x3_to2(xd, wd, bd, add=ad)
    ref.compare(want, ref.conv3x3_to2(x, wt, bias, add), FLOW_BAR, 'aligned')
    assert torch.equal(ops.conv3x3_to2(shifted(xd), wd, bd, add=ad), want)
    assert torch.equal(ops.conv3x3_to2(xd, wd, bd, add=shifted(ad)), want)
    out = shifted(torch.full_like(want, -7.0))
    assert ops.conv3x3_to2(xd, wd, bd, add=ad, out=out) is out and torch.equal(out, want)
    gd = oraft.coords_grid(b, h, w).to(DEV)
    for which in ('flow_out', 'dst1', 'dst2', 'coords_out'):
        hx = shifted(torch.full((b, 256, h, w), -7.0)) if which == 'dst1' else torch.full((b, 256, h, w), -7.0, device=DEV)
        rhx = shifted(torch.full((b, 256, h, w), -7.0)) if which == 'dst2' else torch.full((b, 256, h, w), -7.0, device=DEV)
        flow = shifted(torch.full((b, 2, h, w), -7.0)) if which == 'flow_out' else torch.full((b, 2, h, w), -7.0, device=DEV)
        co = shifted(torch.full((b, 2, h, w), -7.0)) if which == 'coords_out' else torch.full((b, 2, h, w), -7.0, device=DEV)
        assert any(t.data_ptr() % 16 for t in (hx[:, 254:], rhx[:, 254:], flow, co))
        ops.flow_update(xd, wd, bd, ad, co, flow_out=flow, dst1=hx[:, 254:], dst2=rhx[:, 254:])
        assert torch.equal(co, want), which
        for dst in (flow, hx[:, 254:], rhx[:, 254:]):
            assert torch.equal(dst, want - gd), which
        assert bool((hx[:, :254] == -7.0).all()) and bool((rhx[:, :254] == -7.0).all()), which


# ============================================================================================================ element-wise kernels
GATE_BAR, GATE_H_BAR, EPI_BAR = 1e-6, 2e-6, 2e-5           # the bars of test_gru_gates and test_encoder_epilogues
# more than 2048 blocks * 256 threads * VEC elements per batch item: (b, c, h, w)
TRIP_CASES = {'vec4': (1, 130, 128, 128),                 # 2 129 920 > 2 097 152, hw % 4 == 0
              'vec1': (2, 131, 63, 65)}                   # 536 445 > 524 288, hw odd


def _trip(cls):
    b, c, h, w = TRIP_CASES[cls]
    assert c * h * w > 2048 * 256 * (4 if cls == 'vec4' else 1) and ((h * w) % 4 == 0) == (cls == 'vec4')
    return b, c, h, w, torch.Generator().manual_seed(c)


@pytest.mark.parametrize('cls', list(TRIP_CASES))
def test_gates_second_grid_stride_trip(rpe, cls):
    from rpe_amd import ops
    b, c, h, w, g = _trip(cls)
    zr, add = torch.randn(b, 2 * c, h, w, generator=g) * 3, torch.randn(b, 2 * c, h, w, generator=g)
    bias = torch.randn(2 * c, generator=g)
    hx, rh0 = torch.randn(b, c + 3, h, w, generator=g), torch.randn(b, c + 5, h, w, generator=g)
    z_out, rhx = torch.full((b, c, h, w), -7.0, device=DEV), rh0.to(DEV)
    ops.gru_gates_zr(zr.to(DEV), hx.to(DEV), c, z_out, rhx, bias=bias.to(DEV), add=add.to(DEV))
    z_ref, rh_ref = ref.gates_zr(zr, bias, add, hx, c)
    ez, er = ref.compare(z_out, z_ref, GATE_BAR, 'z'), ref.compare(rhx[:, :c], rh_ref, GATE_BAR, 'r*h')
    assert torch.equal(rhx[:, c:].cpu(), rh0[:, c:])                      # the channels behind the slice
    q, qadd, bq = torch.randn(b, c, h, w, generator=g) * 3, torch.randn(b, c, h, w, generator=g), torch.randn(c, generator=g)
    ho0 = torch.randn(b, c + 2, h, w, generator=g)
    h_out = ho0.to(DEV)
    ops.gru_gates_h(z_out, q.to(DEV), hx.to(DEV), c, h_out, bias=bq.to(DEV), add=qadd.to(DEV))
    eh = ref.compare(h_out[:, :c], ref.gates_h(z_out, q, bq, qadd, hx), GATE_H_BAR, 'h')
    assert torch.equal(h_out[:, c:].cpu(), ho0[:, c:])
    print(f'gates {cls}: z {ez:.2e}  r*h {er:.2e}  h {eh:.2e}')


@pytest.mark.parametrize('cls', list(TRIP_CASES))
def test_bias_affine_copy_second_grid_stride_trip(rpe, cls):
    from rpe_amd import ops
    b, c, h, w, g = _trip(cls)
    x, bias = torch.randn(b, c, h, w, generator=g) * 3 + 1, torch.randn(c, generator=g)
    x[0, 0, 0, 0] = x[b - 1, c - 1, h - 1, w - 1] = NAN
    xd = x.to(DEV)
    # bias_act: exactly relu(x + bias) in float32, into two buffers at different channel offsets
    o1, o2 = torch.full((b, c + 7, h, w), 5.0, device=DEV), torch.full((b, c + 4, h, w), 5.0, device=DEV)
    ops.bias_act(xd, bias.to(DEV), relu=True, out=o1, out_offset=3, out2=o2, out2_offset=4)
    want = torch.relu(x + bias[None, :, None, None])
    for buf, off in ((o1, 3), (o2, 4)):
        assert same_bits(buf[:, off:off + c], want)
        assert bool((buf[:, :off] == 5.0).all()) and bool((buf[:, off + c:] == 5.0).all())
    # affine_act with a residual
    scale, shift, res = torch.randn(c, generator=g), torch.randn(c, generator=g), torch.randn(b, c, h, w, generator=g)
    out = torch.full((b, c, h, w), -7.0, device=DEV)
    ops.affine_act(xd, scale.to(DEV), shift.to(DEV), relu=True, residual=res.to(DEV), out=out)
    ea = ref.compare(out, ref.affine_act(x, scale, shift, True, res), EPI_BAR, 'affine_act')
    print(f'affine_act {cls}: {ea:.2e}')
    # copy_planes between channel slices
    src, dst = torch.randn(b, c + 4, h, w, generator=g).to(DEV), torch.full((b, c + 6, h, w), 5.0, device=DEV)
    ops.copy_planes(src[:, 2:2 + c], dst[:, 3:3 + c])
    assert torch.equal(dst[:, 3:3 + c], src[:, 2:2 + c]) and bool((dst[:, :3] == 5.0).all()) and bool((dst[:, 3 + c:] == 5.0).all())


def test_copy_rect_second_grid_stride_trip(rpe):
    from rpe_amd import ops
    b, c, h, w = TRIP_CASES['vec1']
    assert c * h * w > 2048 * 256
    src = torch.randn(b, c, 66, 72, generator=torch.Generator().manual_seed(9)).to(DEV)
    dst = torch.full((b, c, 70, 80), 5.0, device=DEV)
    ops.copy_rect(src, dst, h, w)
    assert torch.equal(dst[:, :, :h, :w], src[:, :, :h, :w])
    assert bool((dst[:, :, h:] == 5.0).all()) and bool((dst[:, :, :, w:] == 5.0).all())


def test_elementwise_misaligned_bases(rpe):
    """hw % 4 == 0 and one base offset by a float: every dispatcher must fall back to its scalar instantiation.  bias_act, affine_act and the
    copies give exactly the aligned call's result; the gates stay within their bars (the two instantiations may contract differently)."""
    from rpe_amd import ops
    g = torch.Generator().manual_seed(12)
    b, c, h, w = 2, 6, 4, 8
    al = lambda t: t.to(DEV)                                               # noqa: E731
    x, bias, res = torch.randn(b, c, h, w, generator=g) * 3, torch.randn(c, generator=g), torch.randn(b, c, h, w, generator=g)
    scale, shift = torch.randn(c, generator=g), torch.randn(c, generator=g)
    fill = lambda *s: torch.full(s, 5.0)                                   # noqa: E731
    # bias_act: x, out1, out2 in turn
    want1, want2 = al(fill(b, c + 2, h, w)), al(fill(b, c + 3, h, w))
    ops.bias_act(al(x), al(bias), relu=True, out=want1, out_offset=1, out2=want2, out2_offset=2)
    assert same_bits(want1[:, 1:1 + c], torch.relu(x + bias[None, :, None, None]))
    for which in range(3):
        mk = [shifted if which == k else al for k in range(3)]
        o1, o2 = mk[1](fill(b, c + 2, h, w)), mk[2](fill(b, c + 3, h, w))
        ops.bias_act(mk[0](x), al(bias), relu=True, out=o1, out_offset=1, out2=o2, out2_offset=2)
        assert torch.equal(o1, want1) and torch.equal(o2, want2), which
    # affine_act: x, residual, out
    want = ops.affine_act(al(x), al(scale), al(shift), relu=True, residual=al(res), out=al(fill(b, c, h, w)))
    ref.compare(want, ref.affine_act(x, scale, shift, True, res), EPI_BAR, 'affine aligned')
    for which in range(3):
        mk = [shifted if which == k else al for k in range(3)]
        got = ops.affine_act(mk[0](x), al(scale), al(shift), relu=True, residual=mk[1](res), out=mk[2](fill(b, c, h, w)))
        assert torch.equal(got, want), which
    # copies: source or destination buffer shifted
    for which in range(2):
        mk = [shifted if which == k else al for k in range(2)]
        src, dst = mk[0](torch.randn(b, c + 2, h, w, generator=g)), mk[1](fill(b, c + 3, h, w))
        ops.copy_planes(src[:, 1:1 + c], dst[:, 2:2 + c])
        assert torch.equal(dst[:, 2:2 + c], src[:, 1:1 + c]) and bool((dst[:, :2] == 5.0).all()) and bool((dst[:, 2 + c:] == 5.0).all())
        dst2 = mk[1](fill(b, c + 2, h + 2, w + 4))
        ops.copy_rect(src, dst2, h - 1, w - 1)
        assert torch.equal(dst2[:, :, :h - 1, :w - 1], src[:, :, :h - 1, :w - 1])
        assert bool((dst2[:, :, h - 1:] == 5.0).all()) and bool((dst2[:, :, :, w - 1:] == 5.0).all())
    # gates: each tensor in turn
    zr, add, bzr = torch.randn(b, 2 * c, h, w, generator=g) * 3, torch.randn(b, 2 * c, h, w, generator=g), torch.randn(2 * c, generator=g)
    hx, rh0 = torch.randn(b, c + 2, h, w, generator=g), torch.randn(b, c + 1, h, w, generator=g)
    q, qadd, bq = torch.randn(b, c, h, w, generator=g) * 3, torch.randn(b, c, h, w, generator=g), torch.randn(c, generator=g)
    z_ref, rh_ref = ref.gates_zr(zr, bias=bzr, add=add, h=hx, c=c)
    for which in range(5):
        mk = [shifted if which == k else al for k in range(5)]
        z_out, rhx = mk[3](fill(b, c, h, w)), mk[4](rh0)
        ops.gru_gates_zr(mk[0](zr), mk[2](hx), c, z_out, rhx, bias=al(bzr), add=mk[1](add))
        ref.compare(z_out, z_ref, GATE_BAR, f'z, misaligned {which}')
        ref.compare(rhx[:, :c], rh_ref, GATE_BAR, f'r*h, misaligned {which}')
        assert torch.equal(rhx[:, c:].cpu(), rh0[:, c:])
        zin = z_ref.float()
        h_out = mk[4](torch.cat([fill(b, c, h, w), rh0[:, :1]], 1))
        ops.gru_gates_h(mk[3](zin), mk[0](q), mk[2](hx), c, h_out, bias=al(bq), add=mk[1](qadd))
        ref.compare(h_out[:, :c], ref.gates_h(zin, q, bq, qadd, hx), GATE_H_BAR, f'h, misaligned {which}')
        assert torch.equal(h_out[:, c:].cpu(), rh0[:, :1])


PRE = [0.0, -0.0, 1e-8, -1e-8, 20.0, -20.0, 87.0, -87.0, 88.8, -88.8, 89.0, -89.0, 104.0, -104.0, 1e4, -1e4, INF, -INF, NAN]
HID = [0.0, 1.0, -1.0, 1e-30, -1e-30]
ZIN = [0.0, 1.0, 0.5, 1e-8, 1.0 - 2.0 ** -24]


@pytest.mark.parametrize('h,w', [(5, 8), (5, 5)])                          # hw % 4 == 0: float4 class; odd: scalar class
@pytest.mark.parametrize('via', ('tensor', 'bias', 'add'))
def test_gate_saturation(rpe, via, h, w):
    """Pre-activations from +-0 over +-88.8 (expf overflows just below) to +-1e4, +-Inf and NaN -- one per channel, brought in through the
    tensor, the bias or ``add`` -- against every hidden-state value of HID: 1e-6 / 2e-6 against float64, z in [0, 1] exactly, NaN only where
    the reference has it."""
    from rpe_amd import ops
    c, n = len(PRE), h * w
    pre = torch.tensor(PRE)
    idx = torch.arange(n)
    hid = torch.tensor(HID)[idx % 5].view(1, 1, h, w)
    hx = torch.cat([hid.expand(1, c, h, w), torch.full((1, 2, h, w), 9.0)], 1).contiguous()

    def place(v, ch):                                                      # (tensor, bias, add) that bring v[k] to channel k
        full = v.view(1, ch, 1, 1).expand(1, ch, h, w).contiguous()
        zero = torch.zeros(1, ch, h, w)
        return {'tensor': (full, None, None), 'bias': (zero, v.clone(), None), 'add': (zero, None, full)}[via]

    zr, bias, add = place(torch.cat([pre, pre]), 2 * c)
    dv = lambda t: None if t is None else t.to(DEV)                        # noqa: E731
    z_out, rhx = torch.full((1, c, h, w), -7.0, device=DEV), torch.full((1, c + 1, h, w), -7.0, device=DEV)
    ops.gru_gates_zr(dv(zr), dv(hx), c, z_out, rhx, bias=dv(bias), add=dv(add))
    z_ref, rh_ref = ref.gates_zr(zr, bias, add, hx, c)
    ref.compare(z_out, z_ref, GATE_BAR, 'z')
    ref.compare(rhx[:, :c], rh_ref, GATE_BAR, 'r*h')
    zc = z_out.cpu()
    assert bool(((zc >= 0.0) & (zc <= 1.0) | torch.isnan(zc)).all()) and bool((rhx[:, c:] == -7.0).all())
    zin = torch.tensor(ZIN)[(idx // 5) % 5].view(1, 1, h, w).expand(1, c, h, w).contiguous()
    q, bq, qadd = place(pre, c)
    h_out = torch.full((1, c + 1, h, w), -7.0, device=DEV)
    ops.gru_gates_h(dv(zin), dv(q), dv(hx), c, h_out, bias=dv(bq), add=dv(qadd))
    ref.compare(h_out[:, :c], ref.gates_h(zin, q, bq, qadd, hx), GATE_H_BAR, 'h')
    assert bool((h_out[:, c:] == -7.0).all())


# ================================================================================================================== instance norm
def torch_f32_instnorm(pre, relu, res):
    """torch's own float32 answer: F.instance_norm (for a one-element plane, which it refuses, the same formula in float32 tensor ops)."""
    if pre.shape[2] * pre.shape[3] == 1:
        y = (pre - pre.mean((2, 3), keepdim=True)) / torch.sqrt(pre.var((2, 3), unbiased=False, keepdim=True) + 1e-5)
    else:
        y = F.instance_norm(pre, eps=1e-5)
    if relu:
        y = torch.relu(y)
    return y if res is None else torch.relu(res + y)


@pytest.mark.parametrize('with_res', (False, True))
@pytest.mark.parametrize('relu', (False, True))
@pytest.mark.parametrize('h,w', [(127, 129), (128, 128), (4, 4097), (1, 1), (1, 3)])
def test_instnorm_plane_classes_and_degenerate_planes(rpe, h, w, relu, with_res):
    """hw = 16383 (256 threads, scalar loads), 16384 and 16388 (512 threads, eight partial sums), 1 and 3.  Channels 0 and 3: N(1, 3) planes at
    the 2e-5 bar of test_encoder_epilogues.  Channel 1: a constant plane (variance 0, invstd = 1/sqrt(eps)); channel 2: mean 1e4, sigma 1.  For
    those two the bar is 4x the error of torch's float32 F.instance_norm on the same input against the same float64 truth.

    Measured (kernel on an MI355X / torch's float32 operator on the CPU), largest over the cases: constant planes 0 (exactly) / 1.1e-5;
    mean-1e4 planes 6.4e-7 / 3.6e-4 to 1.0e-3; one-element planes 0 / 0.  Before the kernel's sums were taken about the plane's first
    value, a float32 model of it gave 2e-5 to 1e-3 on the constant planes and 1.3e-4 to 8.5e-4 on the mean-1e4 planes: 10 to 100x torch's
    error where 4x is allowed."""
    from rpe_amd import ops
    g = torch.Generator().manual_seed(h * w)
    x = torch.randn(2, 4, h, w, generator=g) * 3 + 1
    x[0, 1], x[1, 1] = 0.1, 3.7
    x[:, 2] = torch.randn(2, h, w, generator=g) + 1e4
    bias = torch.tensor([0.3, 0.37, -0.21, 0.0])
    res = torch.randn(2, 4, h, w, generator=g) if with_res else None
    truth = ref.instnorm_act(x, bias, 1e-5, relu, res)
    yard = torch_f32_instnorm(x + bias[None, :, None, None], relu, res)
    got = ops.instnorm_act(x.to(DEV), bias.to(DEV), eps=1e-5, relu=relu, residual=None if res is None else res.to(DEV),
                           out=torch.full((2, 4, h, w), -7.0, device=DEV))
    bad = []
    for ch, kind in ((0, 'plain'), (1, 'constant'), (2, 'mean 1e4'), (3, 'plain')):
        fy = float((yard[:, ch].double() - truth[:, ch]).abs().max())
        bar = EPI_BAR if kind == 'plain' else 4.0 * fy
        try:
            e = ref.compare(got[:, ch], truth[:, ch], bar, kind)
        except AssertionError as err:
            bad.append(str(err))
            e = float((got[:, ch].cpu().double() - truth[:, ch]).abs().max())
        print(f'instnorm {h}x{w} relu={relu} res={with_res} {kind}: hip {e:.3e}   torch f32 {fy:.3e}   bar {bar:.3e}')
    assert not bad, bad


def test_instnorm_refuses_a_misaligned_vector_plane(rpe):
    """hw % 4 == 0 with a base one float into an allocation: RpeError, the output untouched.  With hw odd the same base is fine."""
    from rpe_amd import ops
    g = torch.Generator().manual_seed(5)
    x, res, bias = torch.randn(2, 3, 4, 8, generator=g), torch.randn(2, 3, 4, 8, generator=g), torch.randn(3, generator=g)
    for which in range(3):
        mk = [shifted if which == k else (lambda t: t.to(DEV)) for k in range(3)]
        out = mk[2](torch.full((2, 3, 4, 8), -7.0))
        with pytest.raises(rpe.RpeError):
            ops.instnorm_act(mk[0](x), bias.to(DEV), relu=True, residual=mk[1](res), out=out)
        torch.cuda.synchronize()
        assert bool((out == -7.0).all()), which
    xo, ro = torch.randn(2, 3, 5, 7, generator=g) * 3 + 1, torch.randn(2, 3, 5, 7, generator=g)
    got = ops.instnorm_act(shifted(xo), bias.to(DEV), relu=True, residual=shifted(ro), out=shifted(torch.zeros(2, 3, 5, 7)))
    ref.compare(got, ref.instnorm_act(xo, bias, 1e-5, True, ro), EPI_BAR, 'odd hw, shifted bases')


# ==================================================================================================================== up-sampling
UP_SHAPES = [(1, 1, 1), (1, 1, 300), (1, 300, 1), (2, 17, 23), (3, 33, 9), (1, 16, 16), (1, 16, 17)]
UP_REGIMES = ('sigma2', 'sigma80', 'spikes', 'neg_inf', 'equal', 'pos_inf')


def up_case(b, h8, w8, regime):
    g = torch.Generator().manual_seed(h8 * 1000 + w8 + 7 * UP_REGIMES.index(regime))
    flow = torch.randn(b, 2, h8, w8, generator=g) * 4
    mask = torch.randn(b, 576, h8, w8, generator=g) * (80 if regime == 'sigma80' else 2)
    cell = torch.arange(b * h8 * w8).view(b, 1, h8, w8)
    if regime == 'spikes':                                                 # +1e4 at one channel of every third cell, -1e4 at one of the next
        ch = torch.randint(576, (b, 1, h8, w8), generator=g)
        spike = torch.where(cell % 3 == 0, 1e4, torch.where(cell % 3 == 1, -1e4, 0.0))
        cur = mask.gather(1, ch)
        mask.scatter_(1, ch, torch.where(spike != 0, spike, cur))
    elif regime == 'neg_inf':                                              # some of the nine; all nine of sub-pixel 5 in every second cell
        mask[torch.rand(mask.shape, generator=g) < 0.2] = -INF
        sub5 = mask[:, 5::64]
        sub5[(cell % 2 == 0).expand_as(sub5)] = -INF
    elif regime == 'equal':                                                # nine equal logits per sub-pixel
        mask = (torch.randn(b, 1, 64, h8, w8, generator=g) * 2).expand(b, 9, 64, h8, w8).reshape(b, 576, h8, w8).contiguous()
    elif regime == 'pos_inf':
        mask[torch.rand(mask.shape, generator=g) < 0.02] = INF
        mask[0, 70, 0, 0] = INF
    return flow, mask


def up_errors(flow, mask, got=None):
    """(error of the float32 oracle on the CPU, error of ``got``) against float64 over the elements the truth has finite, both relative to
    max |8 flow| over the finite flow; NaN / Inf positions of ``got`` are checked on the way."""
    truth = ref.upsample_convex(flow, mask)
    scale = float((8 * flow[torch.isfinite(flow)]).abs().max())
    fin = torch.isfinite(truth)
    yard = oraft.upsample_flow(flow, mask).double()
    assert torch.equal(torch.isfinite(yard), fin)
    fy = float((yard[fin] - truth[fin]).abs().max()) / scale if bool(fin.any()) else 0.0
    if got is None:
        return fy, None, truth, scale
    return fy, ref.compare(got, truth, INF, 'positions') / scale, truth, scale


@functools.lru_cache(maxsize=None)
def up_yardstick(regime):
    """The float32 oracle's error in this regime: the largest over UP_SHAPES, relative to max |8 flow|."""
    return max(up_errors(*up_case(*s, regime))[0] for s in UP_SHAPES)


@pytest.mark.parametrize('regime', UP_REGIMES)
@pytest.mark.parametrize('b,h8,w8', UP_SHAPES)
def test_upsample_convex_shapes_and_logit_regimes(rpe, b, h8, w8, regime):
    """One cell, one row, one column, odd maps, exactly one 256-thread block and one cell more, under six logit regimes.  The bar: 4x the
    float32 oracle's error against float64 in the regime (largest over the shapes), relative to max |8 flow| -- the kernel has another expf and
    another order of the nine products.  sigma2 also keeps the 2e-5 absolute bar of test_convex_upsample; with nine equal logits the result
    is also held to the plain mean of the nine zero-padded neighbours.

    Measured, relative to max |8 flow| of about 100 (float32 oracle / kernel, largest over the shapes): sigma2 2.0e-7 / see below,
    sigma80 1.7e-7 / 1.1e-7, spikes 2.7e-7 / 1.8e-7, neg_inf 2.1e-7 / 1.6e-7, equal 3.8e-8 / 1.4e-8, pos_inf 2.6e-7 / 1.9e-7 -- those with
    the softmax in float32.  sigma2 then missed the absolute bar (2.3e-5 at (2,17,23), the float32 oracle itself 2.8e-5; 2.2e-5 at (1,16,17)
    with only the nine products summed in double), so the kernel now evaluates softmax and sum in double and rounds once."""
    from rpe_amd import ops
    flow, mask = up_case(b, h8, w8, regime)
    got = ops.upsample_convex(flow.to(DEV), mask.to(DEV))
    fy, e, truth, scale = up_errors(flow, mask, got)
    bar = 4.0 * up_yardstick(regime)
    print(f'upsample {(b, h8, w8)} {regime}: hip {e:.3e}   f32 oracle here {fy:.3e}, in the regime {bar / 4:.3e}   (relative to {scale:.1f})')
    ref.compare(got, truth, bar * scale, regime)
    if regime == 'sigma2':
        ref.compare(got, truth, 2e-5, 'sigma2, absolute')
    if regime == 'equal':
        mean = F.avg_pool2d(8 * flow.double(), 3, stride=1, padding=1).repeat_interleave(8, 2).repeat_interleave(8, 3)
        ref.compare(got, mean, bar * scale, 'mean of nine')
    if regime in ('neg_inf', 'pos_inf'):
        assert bool(torch.isnan(truth).any())
    if regime not in ('neg_inf', 'pos_inf'):
        assert bool(torch.isfinite(got).all())


@pytest.mark.parametrize('b,h8,w8', [(2, 17, 23), (3, 33, 9)])
def test_upsample_convex_extreme_flow_pixels(rpe, b, h8, w8):
    """+-1e6, Inf and NaN flow pixels, each once inside and once on the border (seen there through a zero-padded neighbourhood), sigma-2
    logits: NaN / Inf exactly where float64 has them, no overflow elsewhere, 4x the float32 oracle's error on this input, and the plain 2e-5
    bar in every cell whose 3x3 neighbourhood holds none of the eight pixels.

    The errors are printed; relative to max |8 flow| = 8e6 the bar is loose, which is why the 2e-5 check of the far cells is there."""
    from rpe_amd import ops
    flow, mask = up_case(b, h8, w8, 'sigma2')
    spots = [(0, 0, 5, 4, 1e6), (0, 1, 0, 3, 1e6), (0, 1, 9, 6, -1e6), (b - 1, 0, h8 - 1, w8 - 1, -1e6),
             (b - 1, 0, 12, 3, INF), (0, 0, 8, 0, INF), (b - 1, 1, 4, 5, NAN), (b - 1, 1, h8 - 1, 2, NAN)]
    far = torch.ones(b, 1, h8, w8, dtype=torch.bool)
    for (i, ch, y, x, v) in spots:
        flow[i, ch, y, x] = v
        far[i, 0, max(0, y - 1):y + 2, max(0, x - 1):x + 2] = False
    got = ops.upsample_convex(flow.to(DEV), mask.to(DEV))
    fy, e, truth, scale = up_errors(flow, mask, got)
    print(f'upsample {(b, h8, w8)} extreme flow: hip {e:.3e}   f32 oracle {fy:.3e}   (relative to {scale:.3e})')
    assert bool(torch.isnan(truth).any()) and bool(torch.isinf(truth).any())
    ref.compare(got, truth, 4.0 * fy * scale, 'extreme flow')
    far = far.repeat_interleave(8, 2).repeat_interleave(8, 3).expand(b, 2, 8 * h8, 8 * w8)
    assert bool(torch.isfinite(truth[far]).all())
    ref.compare(got.cpu()[far], truth[far], 2e-5, 'cells away from the extreme pixels')


def test_upsample_convex_pitched(rpe):
    """rpe_upsample_convex_ex: a 17 x 23 field in 24 x 32 maps whose padding is NaN -- the dense call's bits."""
    from rpe_amd import ops
    b, h8, w8, mh, mw = 2, 17, 23, 24, 32
    flow, mask = up_case(b, h8, w8, 'sigma2')
    fmap, mmap = torch.full((b, 2, mh, mw), NAN), torch.full((b, 576, mh, mw), NAN)
    fmap[:, :, :h8, :w8], mmap[:, :, :h8, :w8] = flow, mask
    got = ops.upsample_convex(fmap.to(DEV), mmap.to(DEV), size=(h8, w8))
    assert tuple(got.shape) == (b, 2, 8 * h8, 8 * w8)
    assert torch.equal(got, ops.upsample_convex(flow.to(DEV), mask.to(DEV)))
    ref.compare(got, ref.upsample_convex(flow, mask), 2e-5, 'pitched')
