"""The yardstick of tests/test_attention_forms_gpu.py, checked on the CPU: the emulator of attn_kernel's rounding points (tests/attention_ref.py) against
the float64 reference, per row and head, on the Gaussian and the structured inputs the GPU tests use -- one case per dtype, head dim and mask form at the
rescale shapes (one query block and one row; four full key tiles and a ragged fifth), B = 2, H = 3.

What it shows: an implementation that carries exactly the documented roundings stays, in its WORST row, inside the bounds the project applies to whole tensors
(2e-3 for f16, 3e-3 for f16 at head dim 128, 2e-2 for bf16).  The GPU tests may therefore bound every single row of the kernel by twice the emulator's
worst row plus one ulp and still be tighter than the whole-tensor bounds.  The measured maxima are printed (pytest -s) and copied into the header of the
GPU test file.

The outlier family (one key = 6 x one query, the construction of test_attention_dh40_outlier_key_takes_the_safe_path) is asserted on the rows the GPU
test names -- the outlier query's row and a row of another wave of its workgroup; its all-rows figure is printed only: to the other queries the 6 x key is
a random direction with scores of sigma 6, a peaky softmax in which the rounding of Q (scale log2 e) to f16 (step 1 of the emulator) moves competing
scores by 2^-11 of their size: 2.1e-3 in the worst row at head dim 40, a property of the documented roundings and not of any kernel."""
import pytest
import torch

from tests import attention_ref as R

B, H = 2, 3
CASES = [(name, fam) for name, (kind, dh, dt, rows, _) in R.FORMS.items() if name != "dh40_qt2"
         for fam in ["gauss", "edge"] + R.rescale_families(kind, dh) + (["outlier"] if dh in (40, 128) and kind == "plain" else [])]


@pytest.mark.parametrize("name,family", CASES)
def test_emulator_rows_stay_inside_the_whole_tensor_bounds(name, family):
    kind, dh, dt, rows, _ = R.FORMS[name]
    Nq, Nk = R.rescale_shape(kind, rows)
    c = R.make_case(kind, dh, dt, B, H, Nq, Nk, family)
    assert torch.isfinite(c.ref).all()
    bound = R.whole_tensor_bound(dh, dt)
    worst = c.emu_max
    if family == "outlier":
        worst = float(c.emu_rows[:, [5, 5 + rows // 4]].max())
    print(f"emulator vs fp64  {name:15s} {family:10s} Nq {Nq} Nk {Nk}: max row err {c.emu_max:.3e}  asserted {worst:.3e}  bound {bound:.0e}")
    assert worst < bound, (worst, bound)


def test_emulator_denominator_follows_the_kernel():
    """head dim 40 sums the rounded P (ones column), every other form the fp32 exponentials (l_run): the two differ, and the default picks by head dim"""
    for dh in (40, 64):
        q, k, v = R.gaussian(1, 2, 33, 70, dh, torch.float16, 5)
        a = R.attention_emulated(q, k, v, 2, dh ** -0.5, denominator="rounded")
        b = R.attention_emulated(q, k, v, 2, dh ** -0.5, denominator="unrounded")
        d = R.attention_emulated(q, k, v, 2, dh ** -0.5)
        assert not torch.equal(a, b)
        assert torch.equal(d, a if dh == 40 else b)


def test_fp64_reference_matches_torch_softmax():
    q, k, v = R.gaussian(2, 3, 17, 17, 64, torch.float16, 9)
    bias = R.bias_tensor(3, 17, 1)
    for causal, bs in ((False, None), (True, None), (False, bias)):
        got = R.attention_fp64(q, k, v, 3, 0.125, causal, bs)
        qh, kh, vh = (t.double().view(2, 17, 3, 64).transpose(1, 2) for t in (q, k, v))
        s = qh @ kh.transpose(-1, -2) * 0.125
        if bs is not None:
            s = s + R.bias_for_abi(bs).double() / R.LOG2E
        if causal:
            s = s + torch.full((17, 17), float("-inf"), dtype=torch.float64).triu(1)
        want = (torch.softmax(s, -1) @ vh).transpose(1, 2).reshape(2, 17, 192)
        assert float((got - want).abs().max()) < 1e-12
