"""GPU: mt_checksum64 (csrc/optim.hip) against the numpy form of the same formula (checkpoint.checksum64_reference).  The values are
64-bit integers: every comparison is exact.  Sizes: one word, less than a vector, the workgroup's 256 threads and one more or fewer,
one workgroup's 4 096 words plus one (two workgroups), and 2^20 + 5 (256 workgroups, grid stride, a tail); pointers 4, 8 and 12 bytes
past a 16-byte boundary (the scalar head); index bases 0, 7 and 2^33 (64-bit positions)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from modaltune_amd import ops  # noqa: E402
from modaltune_amd.checkpoint import as_unsigned, checksum64_reference  # noqa: E402

SIZES = (1, 3, 255, 256, 257, 4096 + 1, (1 << 20) + 5)
PATTERN = 0x5A5A5A5A5A5A5A5A
M64 = (1 << 64) - 1
_data = {}


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _words():
    """One buffer of random words on a 16-byte boundary, on both sides (made once)."""
    if not _data:
        r = np.random.default_rng(11)
        host = r.integers(0, 1 << 32, size=max(SIZES) + 8, dtype=np.uint64).astype(np.uint32)
        dev = torch.from_numpy(host.view(np.int32)).cuda()
        assert dev.data_ptr() % 16 == 0
        _data.update(host=host, dev=dev)
    return _data["host"], _data["dev"]


def _device_checksum(t, nwords, index_base=0, slack=3):
    """mt_checksum64 into the middle of a patterned int64 tensor, over a patterned workspace with `slack` slots to spare; asserts
    that nothing but out[0] and the used slots was written."""
    used = ops.checksum64_partials_elems(nwords)
    ws = torch.full((used + slack,), PATTERN, dtype=torch.int64, device="cuda")
    out = torch.full((3,), PATTERN, dtype=torch.int64, device="cuda")
    ops.checksum64(t, nwords, ws, out[1:2], index_base=index_base)
    torch.cuda.synchronize()
    assert out[0].item() == PATTERN and out[2].item() == PATTERN
    assert ws[used:].tolist() == [PATTERN] * slack
    return as_unsigned(out[1].item()), used


@pytest.mark.parametrize("nwords", SIZES)
def test_checksum_matches_the_reference_at_every_size_offset_and_base(nwords):
    _gpu()
    host, dev = _words()
    for off in (0, 1, 2, 3):          # words past the 16-byte boundary: 0, 4, 8, 12 bytes
        for base in (0, 7, 1 << 33):
            got, used = _device_checksum(dev[off:off + nwords], nwords, base)
            assert got == checksum64_reference(host[off:off + nwords], index_base=base), (nwords, off, base)
    assert used == min(2048, (nwords + 4095) // 4096) == ops.checksum64_partials_elems(nwords)


def test_pieces_compose_on_the_device_and_float_buffers_are_their_words():
    _gpu()
    host, dev = _words()
    n = 4096 + 1
    whole, _ = _device_checksum(dev[:n], n)
    for k in (1, 259, 4096):
        a, _ = _device_checksum(dev[:k], k)
        b, _ = _device_checksum(dev[k:n], n - k, index_base=k)
        assert (a + b) & M64 == whole, k
    f = torch.randn(1001, device="cuda")
    f[7], f[8] = 0.0, -0.0          # (+0 and -0 are different words)
    got, _ = _device_checksum(f, f.numel())
    assert got == checksum64_reference(f.cpu())
    g = f.clone()
    g[8] = 0.0
    assert _device_checksum(g, g.numel())[0] != got
    z = torch.zeros(300, dtype=torch.int32, device="cuda")
    assert _device_checksum(z, 299)[0] != _device_checksum(z, 300)[0]


def test_bad_arguments_are_refused():
    _gpu()
    host, dev = _words()
    out = torch.zeros(1, dtype=torch.int64, device="cuda")
    ws = torch.zeros(1, dtype=torch.int64, device="cuda")
    with pytest.raises(RuntimeError, match="bad argument"):
        ops.checksum64(dev, 4096 + 1, ws, out)          # two workgroups need two slots
    with pytest.raises(RuntimeError, match="bad argument"):
        ops.checksum64(dev, 0, ws, out)
    assert ops.checksum64_partials_elems(0) < 0 and ops.checksum64_partials_elems(1 << 40) == 2048
