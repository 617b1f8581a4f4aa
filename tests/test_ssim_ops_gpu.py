"""diffusion_nlc_amd.metrics.ssim3d (nlc_ssim3d, csrc/ssim.hip) against the float64 closed form of tests/ssim_refs.py, within
the gate measured on the reference's f32 arithmetic (4 x E32; the flat case, where the cancellation is everything, has the wide one,
every case with texture the tight one - ssim_refs.gate_of).  Shapes: smaller than the halo, equal to it, tile multiples, tile
boundaries inside, the workload's 256 x 256 once, C = 1 / 2 / 4, N = 1 / 2 / 5 and P < N.  Contents: noisy copies, unrelated
pairs, identical pairs, flat images, both branches of max_value, the half-way quantisation grid."""
import pytest
import torch

from tests import ssim_refs as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _gpu(name):
    from diffusion_nlc_amd import metrics
    sample, orig, want = S.case(name)
    got = metrics.ssim3d(sample.to(DEV), orig.to(DEV))
    assert got.dtype == torch.float64 and got.shape == (sample.shape[0],) and got.device == torch.device(DEV)
    return got.cpu(), want


@pytest.mark.parametrize("name", list(S.CASES))
def test_ssim3d_matches_the_closed_form(name):
    got, want = _gpu(name)
    err = (got - want).abs().max().item()
    print(f"{name}: ssim64 {want[0].item():+.9f}, |kernel - ssim64| {err:.3e}, gate {S.gate_of(name):.3e}")
    assert err <= S.gate_of(name)


def test_identical_images_give_one():
    got, _ = _gpu("same_40x70")
    assert abs(got.item() - 1.0) <= S.GATE_TEXTURED


def test_max_value_branches_differ():
    dim, _ = _gpu("dim_40x70")
    bright, _ = _gpu("dim_one_bright_40x70")
    assert abs(dim.item() - bright.item()) > 4 * S.GATE_TEXTURED


def test_fewer_originals_than_samples_is_bit_equal_to_repeated_originals():
    from diffusion_nlc_amd import metrics
    sample, orig, want = S.case("noisy_p2_n6")
    assert sample.shape[0] == 6 and orig.shape[0] == 2
    s, o = sample.to(DEV), orig.to(DEV)
    shared = metrics.ssim3d(s, o)
    repeated = metrics.ssim3d(s, o.repeat(3, 1, 1, 1).contiguous())
    assert torch.equal(shared, repeated)
    for n in range(6):                                            # pair by pair: sample n alone against its own original
        assert torch.equal(metrics.ssim3d(s[n:n + 1], o[n % 2:n % 2 + 1]), shared[n:n + 1])
    assert (shared.cpu() - want).abs().max().item() <= S.GATE_TEXTURED


def test_repeatable_bits_and_cached_workspace():
    """Two calls on one input return identical bits; a call with another N between them (its own workspace, then the cached one
    again) is correct and disturbs nothing."""
    from diffusion_nlc_amd import metrics
    sample, orig, want = S.case("noisy_33x17")
    s, o = sample.to(DEV), orig.to(DEV)
    first = metrics.ssim3d(s, o)
    fewer = metrics.ssim3d(s[:2].contiguous(), o[:2].contiguous())
    again = metrics.ssim3d(s, o)
    assert torch.equal(first, again) and torch.equal(fewer, first[:2])
    assert (fewer.cpu() - want[:2]).abs().max().item() <= S.GATE_TEXTURED
    assert len([k for k in metrics._workspaces if k[2:] == (3, 33, 17)]) == 2


def test_rejects_what_it_would_have_to_move_or_copy():
    from diffusion_nlc_amd import metrics
    from diffusion_nlc_amd._ext import NlcError
    x = torch.rand(2, 3, 8, 12)
    d = x.to(DEV)
    for bad in ((x, d), (d, x), (d.double(), d.double()), (d.transpose(2, 3), d.transpose(2, 3)), (d[:, :, :, ::2], d[:, :, :, ::2]),
                (d, d[:, :2].contiguous()), (d, torch.cat([d, d[:1]])), (d[0], d[0]),
                (torch.rand(1, 5, 8, 8, device=DEV), torch.rand(1, 5, 8, 8, device=DEV))):
        with pytest.raises(NlcError):
            metrics.ssim3d(*bad)
