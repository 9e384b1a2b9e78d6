"""The seven units of the packed band kernel (miniwfa_amd/csrc/mwf_band2_dispatch.h) together: on the device side no kernel is in two objects, and what the seven
hold is what the five matrices declare plus the table form's four and the 4-bit form's nine kernels — nothing more."""
import os

import band_matrix as bm
import band_deep_matrix as dm
import band_biased_matrix as xm
from miniwfa_amd import api as mw
from miniwfa_amd import build as mwbuild

KERNEL_OF_UNIT = {"mwf_band2_tab.hip": "wfa_band2_tab_kernel", "mwf_band2_nib.hip": "wfa_band2_nib_kernel"}   # (every other unit: wfa_band2_kernel)


def test_units_are_disjoint_and_hold_what_is_declared():
    mw.lib()
    assert len(mwbuild.BAND2_UNITS) == 7
    held = {}
    for unit in mwbuild.BAND2_UNITS:
        kernel = KERNEL_OF_UNIT.get(unit, "wfa_band2_kernel")
        got = bm.device_kernels(os.path.join(mwbuild.CSRC, "build", unit + ".o"), kernel)
        assert not isinstance(got, str), got
        insts, others = got
        assert not others, (unit, sorted(others))
        held[unit] = {(kernel, i) for i in insts}
    units = sorted(held)
    for n, a in enumerate(units):
        for b in units[n + 1:]:
            assert not (held[a] & held[b]), (a, b, sorted(held[a] & held[b]))
    declared = {("wfa_band2_kernel", i) for i in bm.declared_instantiations() | dm.declared_instantiations(3) | dm.declared_instantiations(4)
                | xm.declared_instantiations("bi") | xm.declared_instantiations("bi_deep")}
    declared |= {("wfa_band2_tab_kernel", bm.Inst(512, k, 2, 1, tb, 1, 0, 1)) for k in (3, 4) for tb in (0, 1)}
    declared |= {("wfa_band2_nib_kernel", bm.Inst(T, K, 2, 1, tb, 1, 0, fold)) for T, K in ((512, 3), (512, 4), (1024, 5)) for tb, fold in ((1, 0), (0, 1), (0, 0))}
    union = set().union(*held.values())
    assert union == declared, (sorted(union - declared), sorted(declared - union))
    assert sum(len(v) for v in held.values()) == len(declared) == 62 + 28 + 14 + 12 + 12 + 4 + 9
