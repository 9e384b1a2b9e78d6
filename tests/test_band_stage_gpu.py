"""The table form's every-penalty tail (mwf_band2_kernel.h, kChain / kLeanTail: the iteration budget counted down, the end column's chunk marked in `est`, the flag word
written where its bits arise, read early behind the barrier) on the inputs of tests/band_stage_cases.py, whose properties tests/test_band_stage_cpu.py asserts.
Geometry forced to 512 threads on three and on four chunk slots, score-only and with CIGAR: s, n_iter and the CIGAR words equal the oracle's and, bit for bit,
those of the same align with "probe_table" 0 (the plain form keeps the counter and the three compares); one launch, no pair handed back."""
import pytest

import band_stage_cases as sc
from test_band_chain_gpu import both_forms

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("flag", [0, 1], ids=["score", "cigar"])
@pytest.mark.parametrize("slots", [3, 4])
@pytest.mark.parametrize("label", sc.BUDGET_LABELS)
def test_budget(label, slots, flag, oracle, capfd, monkeypatch):
    monkeypatch.setenv("MWF_DEBUG", "1")
    pair, s_star, _, cases = sc.budget_cases(oracle)
    kw = dict(max_iter=dict(cases)[label])
    exp = sc.expected(oracle, "budget", **kw)
    assert (exp[0][0] == -1) == (label != "big")
    both_forms([pair], exp, slots, flag, capfd, f"budget {label} at {s_star} slots {slots} flag {flag}", stopped=label != "big", **kw)


@pytest.mark.parametrize("flag", [0, 1], ids=["score", "cigar"])
@pytest.mark.parametrize("slots", [3, 4])
def test_end_column_in_every_slot(slots, flag, oracle, capfd, monkeypatch):
    monkeypatch.setenv("MWF_DEBUG", "1")
    g = sc.G3 if slots == 3 else sc.G4
    keep = [i for i, ((t, q), (lohi, far)) in enumerate(zip(sc.endslot_group(), sc.traces(oracle))) if sc.fits(lohi, far, t, q, g)]
    assert len(keep) >= 4 and (slots == 3 or len(keep) == len(sc.endslot_group()))
    pairs, exp = [sc.endslot_group()[i] for i in keep], [sc.expected(oracle, "endslot")[i] for i in keep]
    both_forms(pairs, exp, slots, flag, capfd, f"endslot slots {slots} flag {flag}")
