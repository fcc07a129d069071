"""CPU: the duplicate search's report on the loaded library (option dedupe_report, SQYAMD_Dedupe_Report: include/sqeazy_amd.h).  No GPU:
with no call made there is no record, and nothing is written."""
import ctypes


def test_dedupe_report_option_and_empty_read(sqy):
    L = sqy.lib()
    assert sqy.get_option("dedupe_report") == 0                                  # off by default: a call pays one relaxed load
    assert L.SQYAMD_Set_Option(b"dedupe_report", 2) == 1 and L.SQYAMD_Set_Option(b"dedupe_report", -1) == 1
    assert sqy.get_option("dedupe_report") == 0
    with sqy.option("dedupe_report", 1):
        assert sqy.get_option("dedupe_report") == 1
        keys, dup_of = sqy.dedupe_report()
        assert keys.size == 0 and dup_of.size == 0
        fn = L.SQYAMD_Dedupe_Report
        fn.restype = ctypes.c_long
        fn.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.POINTER(ctypes.c_uint), ctypes.c_long]
        gk, gd = (ctypes.c_ulonglong * 4)(*([7] * 4)), (ctypes.c_uint * 4)(*([7] * 4))
        assert fn(None, None, 5) == 0 and fn(gk, gd, 4) == 0 and fn(gk, gd, 0) == 0 and fn(gk, gd, -1) == 0 and fn(gk, None, 4) == 0
        assert list(gk) == [7] * 4 and list(gd) == [7] * 4
    assert sqy.get_option("dedupe_report") == 0
