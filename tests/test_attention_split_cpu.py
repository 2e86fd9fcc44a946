"""CPU checks of the inputs that tests/test_attention_split_gpu.py feeds the split-arithmetic attention kernels with no tolerance
(tests/attention_split_model.py): they are exactly summable at K = 64, and they would expose a lost or mis-paired bf16 plane."""
import pytest
import torch

import attention_split_model as S
import exact as X


@pytest.mark.parametrize("n", S.EXACT_N)
@pytest.mark.parametrize("cls", X.CLASSES)
def test_exact_inputs_are_exactly_summable(cls, n):
    """The fp32 CPU q @ k^T equals the fp64 product -- for every (query, key) pair, not only the attended one -- and so do the scaled
    scores the kernels store as lse; the six kept products reproduce it."""
    c = S.exact_case(cls, n)
    s32 = torch.matmul(c["q"], c["k"].transpose(1, 2))
    s64 = torch.matmul(c["q"].double(), c["k"].double().transpose(1, 2))
    assert torch.equal(s32.double(), s64), "q @ k^T is not exact in fp32"
    budget = torch.matmul(c["q"].double().abs(), c["k"].double().abs().transpose(1, 2)).max().item() / c["unit"]
    assert budget < 2 ** 24, f"sum of |products| = {budget:.0f} units: a partial sum may round"
    att = S.attended_scores(c)
    assert torch.equal(att.double(), S.attended_scores(c, torch.float64))
    assert torch.equal((att * 0.125).double(), att.double() / 8), "score / 8 must be exact"
    assert torch.equal(S.six_term_scores(c), att.double()), "the six kept products must give the exact score"
    assert att.abs().max() > 0 and (att * 0.125).min() > -1e6, "attended scores must stay above the -1e7 of the padded keys"
    dv = c["dO"].sum(1)
    assert torch.equal(dv.double(), c["dO"].double().sum(1)), "sum_q dO is not exact in fp32"
    assert all((p != 0).any() for p in X.split3(c["v"])), "v must fill all three planes"


@pytest.mark.parametrize("n", S.EXACT_N)
@pytest.mark.parametrize("ij,cls", sorted(X.PROVES.items()))
def test_each_product_is_proven_by_its_class(ij, cls, n):
    """Dropping product (plane of q, plane of k) from the model changes the attended scores of the class that proves it."""
    c = S.exact_case(cls, n)
    full, dropped = S.six_term_scores(c), S.six_term_scores(c, drop=ij)
    assert not torch.equal(full, dropped), f"class {cls} does not see product {ij}"
    changed = (full != dropped).double().mean().item()
    assert changed > 0.25, f"class {cls}: only {changed:.2f} of the attended scores depend on product {ij}"
