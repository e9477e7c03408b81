"""tests/native/corecheck.cpp (csrc/wt_dwt_core.h compiled for the host) built as a shared library
and loaded through ctypes: shared by tests/test_core_index.py and tests/test_special_values_ref.py."""
import ctypes
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "_build", "libcorecheck.so")
SRC = os.path.join(HERE, "native", "corecheck.cpp")
HDR = os.path.join(HERE, "..", "wavelettransforms_amd", "csrc", "wt_dwt_core.h")


def load():
    os.makedirs(os.path.dirname(SO), exist_ok=True)
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", SO, SRC])
    return ctypes.CDLL(SO)


def fptr(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
