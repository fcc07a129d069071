"""CPU: the call stamps' option and read-out on the loaded library (call_stamps, SQYAMD_Call_Stamps: include/sqeazy_amd.h).  No GPU: with
no call made there is nothing to give, and nothing is written."""
import ctypes


def test_call_stamp_option_and_empty_read(sqy):
    L = sqy.lib()
    assert sqy.get_option("call_stamps") == 0                                    # off by default: a call pays one relaxed load
    assert L.SQYAMD_Set_Option(b"call_stamps", 2) == 1 and L.SQYAMD_Set_Option(b"call_stamps", -1) == 1
    with sqy.option("call_stamps", 1):
        assert sqy.get_option("call_stamps") == 1
        assert sqy.call_stamps() == []
        L.SQYAMD_Call_Stamps.restype = ctypes.c_long
        L.SQYAMD_Call_Stamps.argtypes = [ctypes.POINTER(ctypes.c_long), ctypes.c_long]
        guard = (ctypes.c_long * 12)(*([-7] * 12))
        assert L.SQYAMD_Call_Stamps(None, 5) == 0 and L.SQYAMD_Call_Stamps(guard, 1) == 0 and L.SQYAMD_Call_Stamps(guard, -1) == 0
        assert list(guard) == [-7] * 12
    assert sqy.get_option("call_stamps") == 0
    assert len(sqy.CALL_STAMP_FIELDS) == 10 and sqy.CALL_STAMP_FIELDS[:3] == ("seq", "lane", "thread")
