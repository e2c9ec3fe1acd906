"""tools/placement_census.py: the census arithmetic on hand-made wave records (no GPU, no binary)."""
import importlib.util
import io
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("placement_census", os.path.join(ROOT, "tools", "placement_census.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _wave(wg, wave, cu, simd, t0=0, t1=1000):
    return dict(wg=wg, wave=wave, xcc=0, se=0, sh=0, cu=cu, simd=simd, slot=0, t0=t0, t1=t1)


def _ten(wg, cu, first_simd, **kw):
    """a ten-wave workgroup dealt round-robin over the four SIMDs from first_simd on"""
    return [_wave(wg, w, cu, (first_simd + w) % 4, **kw) for w in range(10)]


def _census(rows, n_cus, waves):
    out = io.StringIO()
    _tool().census("case", rows, n_cus, waves, out)
    return out.getvalue()


def test_peak_counts_only_what_is_open_at_once():
    peak = _tool().peak
    assert peak([(0, 10), (5, 15), (10, 20)]) == 2      # an interval that ends where the next begins does not overlap it
    assert peak([(0, 10), (1, 9), (2, 8)]) == 3
    assert peak([(0, 1)]) == 1


def test_two_workgroups_one_simd_apart_stack_6_5_5_4():
    rows = _ten(0, cu=3, first_simd=0) + _ten(256, cu=3, first_simd=1)
    txt = _census(rows, n_cus=2, waves=10)
    assert "0,4,8 / 1,5,9 / 2,6 / 3,7: 2" in txt
    assert "2 workgroup(s) 6-5-5-4: 1" in txt
    assert "workgroups per CU (resident at once, peak):                0: 1  2: 1" in txt
    assert "waves per SIMD (resident at once, peak; SIMDs with n waves): 0: 4  4: 1  5: 2  6: 1" in txt
    assert "every wave was resident at once" in txt


def test_aligned_workgroups_stack_6_6_4_4_and_shifted_by_two_interleave():
    assert "2 workgroup(s) 6-6-4-4: 1" in _census(_ten(0, 0, 0) + _ten(1, 0, 0), 1, 10)
    assert "2 workgroup(s) 5-5-5-5: 1" in _census(_ten(0, 0, 0) + _ten(1, 0, 2), 1, 10)


def test_a_second_round_on_the_same_cu_is_not_counted_as_resident():
    rows = _ten(0, 0, 0, t0=0, t1=1000) + _ten(1, 0, 0, t0=2000, t1=3000)
    txt = _census(rows, 1, 10)
    assert "workgroups per CU (CUs with n workgroups over the launch): 0: 0  2: 1" in txt
    assert "workgroups per CU (resident at once, peak):                0: 0  1: 1" in txt
    assert "NOT all resident at once" in txt
    assert "2 workgroup(s) 3-3-2-2: 1" in txt


def test_end_time_by_class_separates_loaded_simds():
    rows = [_wave(0, w, 0, 0, t1=3000) for w in range(3)] + [_wave(0, 3, 0, 1, t1=1000)]
    txt = _census(rows, 1, 4)
    assert "1 wave(s) on the SIMD:     1 waves, duration   1.00 /   1.00, end   1.00 /   1.00" in txt
    assert "3 wave(s) on the SIMD:     3 waves, duration   3.00 /   3.00, end   3.00 /   3.00" in txt
