"""CPU-side checks of the band-kernel matrix (tests/band_matrix.py): its entries are exactly the instantiations of wfa_band2_kernel in the built
object, and the inputs of every cell hold what tests/test_band_matrix_gpu.py relies on — sized from the oracle alone, before any GPU time is spent."""
import pytest

import miniwfa_amd as mw
import band_matrix as bm


def test_matrix_equals_the_instantiations_in_the_object():
    """Adding, removing or re-parameterising an instantiation without its matrix entry fails here and names it."""
    mw.lib()   # (builds the library, and with it the object, where that has not happened yet)
    built = bm.object_instantiations()
    if isinstance(built, str):
        pytest.skip(built)
    declared = bm.declared_instantiations()
    assert len(declared) == len(bm.MATRIX), "an instantiation is listed twice"
    missing = sorted(bm.inst_id(i) for i in built - declared)
    stale = sorted(bm.inst_id(i) for i in declared - built)
    assert not missing and not stale, f"instantiations without a matrix entry: {missing}; matrix entries without an instantiation: {stale}"


def test_symbol_parser_reads_all_eight_arguments():
    built = bm.object_instantiations()
    if isinstance(built, str):
        pytest.skip(built)
    assert built and all(len(i) == 8 and i.T in (64, 128, 256, 512, 768, 1024) and i.TB in (0, 1) and i.FOLD in (0, 1) for i in built)


def test_admission_windows_follow_the_planner():
    """One formula over T and K (mwf_plan.cpp kBand*Window): the eight windows of 64 x 3 ... 1024 x 5."""
    got = sorted({bm.admission_window(g) for g in bm.GEOMS.values()})
    assert got == [448, 1216, 2752, 5824, 7872, 9920, 11968, 20160], got


def test_fold_edge_penalty_sets_sit_on_the_edge():
    last, first = bm.PEN["lag_last_fold"], bm.PEN["lag_first_nofold"]
    assert last["o1"] + last["e1"] == bm.FOLD_MAX_LAG - 1 and bm.pen_folds(last)
    assert first["o1"] + first["e1"] == bm.FOLD_MAX_LAG and not bm.pen_folds(first) and first["o1"] == first["x"]


def test_every_cell_has_its_inputs(oracle, capsys):
    """Group sizes, the pair within a chunk of the (tightened) admission limit, the kinds of pairs, and the share of width-fit candidates the hand-back
    rules drop (at most a quarter), for every run of every cell."""
    lines = []
    bm.self_check(oracle, log=lines.append)
    with capsys.disabled():
        print()
        for ln in sorted(set(lines)):
            print("   " + ln)
