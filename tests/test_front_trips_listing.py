"""The listing check of the read loop's front end (scripts/front_trips_listing.py): in the UNI, the PLAIN and the generic <160,64,256>
compact instantiation of classify_kernel the first record is waited for before the loop, and no wait on the vector-memory counter
lies between the next record's load and the loads of the tail entries; in all three the first such wait is the tail entries'
consumer, behind pass 1 of the two full chunks.  Only that wait instruction and the load mnemonics are looked at.  Needs
no GPU: the built kernels.o is disassembled (without one that is newer than its sources, hipcc builds the assembly of kernels.hip,
which takes minutes)."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _script():
    spec = importlib.util.spec_from_file_location("front_trips_listing", os.path.join(ROOT, "scripts", "front_trips_listing.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def listing():
    mod = _script()
    if mod.hipcc() is None:
        pytest.skip("no hipcc here")
    return mod, mod.listing()


@pytest.mark.parametrize("name", ["UNI", "PLAIN", "generic"])
def test_no_wait_between_the_prefetch_and_the_tail_consumer(listing, name):
    mod, text = listing
    ok, msg = mod.check(mod.body(text, mod.KERNELS[name]))
    print(name, msg)
    assert ok, msg


def test_the_check_tells_the_two_forms_apart():
    """The parent's form of the loop head (the load under `more`, the wait in front of the length's read-first-lane) fails, the new one
    passes: two hand-made instruction lists in the listing's mnemonics."""
    mod = _script()
    pad = ["v_nop"] * 120
    old = ["global_load_dword v6, v1, s[4:5]", "global_load_dword v50, v1, s[6:7]", "s_waitcnt vmcnt(0)"] + pad + \
          ["global_load_dwordx4 v[14:17], v[8:9], off", "global_load_dwordx2 v[8:9], v[8:9], off", "s_waitcnt vmcnt(0)"]
    new = ["global_load_dword v6, v1, s[4:5]", "s_waitcnt vmcnt(0)", "global_load_dword v50, v1, s[6:7]",
           "global_load_dwordx4 v[14:17], v[8:9], off", "global_load_dwordx2 v[8:9], v[8:9], off"] + pad + ["s_waitcnt vmcnt(0)"]
    assert not mod.check(old)[0]
    assert mod.check(new)[0]
    assert not mod.check(new[:5] + pad[:50] + ["s_waitcnt vmcnt(0)"])[0]   # the tail entries consumed too early
