"""GPU: the eight convolution weight packers write the same bytes as the digests recorded in tests/golden/conv_pack_digests.json.

The weights come from integer arithmetic (no RNG), the destination is zero-filled at the queried size, and the sha256 of the packed bytes
is compared.  Shapes (cout, cin) are the smallest that cover a padded cout tile (40), the 32-channel remainder (96) and a ragged cin step
(20, for the packers that take one).  `python tests/test_gpu_conv_pack_bits.py OUT.json` rewrites the recorded digests from the library
in use (RPE_HIP_LIBRARY selects another build)."""
import hashlib
import json
import os
import sys

import pytest
import torch

GOLDEN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'conv_pack_digests.json')

# (pack entry, size query, size unit in bytes, taps per (co, ci), extra leading size arguments (kh, kw), shapes)
SQUARE, ROW5, ONE = ((96, 32), (40, 16)), ((96, 32), (40, 16)), ((96, 20), (40, 16))
PACKERS = [
    ('rpe_conv_wino_pack', 'rpe_conv_wino_packed_floats', 4, 9, (), SQUARE),
    ('rpe_conv_wino24_pack', 'rpe_conv_wino24_packed_floats', 4, 9, (), SQUARE),
    ('rpe_conv_wino_x3_pack', 'rpe_conv_wino_x3_packed_bytes', 1, 9, (), SQUARE),
    ('rpe_conv_wino1d_pack', 'rpe_conv_wino1d_packed_floats', 4, 5, (), ROW5),
    ('rpe_conv_wino1d_x3_pack', 'rpe_conv_wino1d_x3_packed_bytes', 1, 5, (), ROW5),
    ('rpe_conv1x1_pack', 'rpe_conv1x1_packed_floats', 4, 1, (), ONE),
    ('rpe_conv1x1_x3_pack', 'rpe_conv1x1_x3_packed_bytes', 1, 1, (), ONE),
    ('rpe_conv_pack', 'rpe_conv_packed_floats', 4, 9, (3, 3), ((96, 20),)),
    ('rpe_conv_pack', 'rpe_conv_packed_floats', 4, 5, (1, 5), ((96, 20),)),
]
CASES = [(pack, query, unit, taps, khw, cout, cin) for pack, query, unit, taps, khw, shapes in PACKERS for cout, cin in shapes]


def _key(pack, khw, cout, cin):
    return f'{pack}/{cout}x{cin}' + ''.join(f'x{k}' for k in khw)


def _weights(n):
    i = torch.arange(n, dtype=torch.int64)
    return (((i * 2654435761) % 2 ** 32).double() / 2 ** 32 - 0.5).float() * 0.1


def pack_digest(L, pack, query, unit, taps, khw, cout, cin):
    size = getattr(L, query)(cout, cin, *khw) * unit
    assert size > 0 and size % 4 == 0
    w = _weights(cout * cin * taps).cuda()
    dst = torch.zeros(size // 4, dtype=torch.float32, device='cuda')
    assert getattr(L, pack)(w.data_ptr(), cout, cin, *khw, dst.data_ptr(), None) == 0
    torch.cuda.synchronize()
    return hashlib.sha256(dst.cpu().numpy().tobytes()).hexdigest()


@pytest.fixture(scope='module')
def recorded():
    with open(GOLDEN_FILE) as f:
        return json.load(f)


@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES, ids=lambda c: _key(c[0], c[4], c[5], c[6]))
def test_packed_weights_match_recorded_digest(rpe, recorded, case):
    pack, _, _, _, khw, cout, cin = case
    assert pack_digest(rpe.lib(), *case) == recorded[_key(pack, khw, cout, cin)]


if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import rpe_amd
    out = {_key(c[0], c[4], c[5], c[6]): pack_digest(rpe_amd.lib(), *c) for c in CASES}
    with open(sys.argv[1], 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(out, indent=1, sort_keys=True))
