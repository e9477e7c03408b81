"""CPU check of the one-launch small path's tap order and window slots (csrc/small_taps.h, compiled
for the host): over test_small_geom.py's sweep of line lengths, filter lengths, levels and tile
sizes, the kernel's general walk and its fast form must give, bit for bit, wt_ana_point's and
wt_syn_pass's sums, read every tap inside the tile's window, and sm_divmod must agree with / and %
(tests/native/smalltaps.cpp)."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(HERE, "_build", "smalltaps")
CSRC = os.path.join(HERE, "..", "wavelettransforms_amd", "csrc")


def test_small_taps_order_and_slots():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    src = os.path.join(HERE, "native", "smalltaps.cpp")
    deps = [src] + [os.path.join(CSRC, h) for h in ("small_taps.h", "small_geom.h", "wt_dwt_core.h")]
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", EXE, src])
    out = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:]
    assert out.stdout.strip().endswith("0 failing")
