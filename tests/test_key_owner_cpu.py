"""CPU checks of shk_key_owner, the host-only statement of which owner share the engine gives a canonical k-mer: against
a pure-Python restatement of mix_key's top bits written from the constants in include/shk.h's description and
sharkmer_amd/csrc/shk_mix.h (one odd multiplier mod 2^2k: 0xC2B2AE35 up to 42 key bits, 0x9E3779B97F4A7C15 beyond), the
range, a sanity band on how evenly random keys spread, and the arguments it refuses.  No GPU: the function touches no
device."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIX_M32, MIX_M64, MIX_NARROW_BITS = 0xC2B2AE35, 0x9E3779B97F4A7C15, 42
NONE = 0xFFFFFFFF
N_KEYS = 100_000
KEY_SEED = 20261020  # (fixed after the restatement below was seen inside the band for every (k, W) at this seed)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from sharkmer_amd.engine import lib_path
    L = ctypes.CDLL(lib_path())
    L.shk_key_owner.restype = ctypes.c_uint32
    L.shk_key_owner.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64]
    return L


def owners_py(k, w, keys):
    """The top log2(w) bits of (key · M) mod 2^2k, on numpy uint64 (whose product wraps mod 2^64, a multiple of 2^2k)."""
    bits = 2 * k
    m = np.uint64(MIX_M32 if bits <= MIX_NARROW_BITS else MIX_M64)
    mask = np.uint64((1 << bits) - 1)
    with np.errstate(over="ignore"):
        mixed = (keys * m) & mask
    return (mixed >> np.uint64(bits - (w.bit_length() - 1))).astype(np.uint32)


def random_keys(k):
    rng = np.random.default_rng([KEY_SEED, k])
    return rng.integers(0, 1 << (2 * k), size=N_KEYS, dtype=np.uint64)


def test_exported_and_declared(lib):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "shk.h")).read(), flags=re.S)
    assert hasattr(lib, "shk_key_owner")
    assert re.search(r"uint32_t\s+shk_key_owner\s*\(\s*uint32_t k,\s*uint32_t n_owners,\s*uint64_t canonical_kmer\s*\)", hdr)
    assert "#define SHK_FLAG_GROUP_GRAPH 32u" in hdr and "#define SHK_ABI_VERSION 2" in hdr
    mix = open(os.path.join(ROOT, "sharkmer_amd", "csrc", "shk_mix.h")).read()
    assert "0x%Xull" % MIX_M32 in mix and "0x%Xull" % MIX_M64 in mix and "SHK_MIX_NARROW_BITS %d" % MIX_NARROW_BITS in mix
    # one place: the device header takes them from there
    assert "#define SHK_MIX_M32 " not in open(os.path.join(ROOT, "sharkmer_amd", "csrc", "shk_device.hip.h")).read()


@pytest.mark.parametrize("k", [1, 11, 15, 21, 22, 31])
def test_one_owner_owns_everything(lib, k):
    for x in random_keys(k)[:1000].tolist() + [0, (1 << (2 * k)) - 1]:
        assert lib.shk_key_owner(k, 1, x) == 0


def test_the_restatement_spreads_random_keys_evenly():
    """The band the library is held to below, on the Python restatement alone: a sanity check, not a measurement."""
    for k in (11, 15, 21, 22, 31):
        for w in (2, 8, 64):
            share = np.bincount(owners_py(k, w, random_keys(k)), minlength=w) / N_KEYS
            assert share.min() >= 0.8 / w and share.max() <= 1.2 / w, (k, w, share.min() * w, share.max() * w)


@pytest.mark.parametrize("w", [2, 8, 64])
@pytest.mark.parametrize("k", [11, 15, 21, 22, 31])
def test_owner_is_the_top_of_the_mixed_key(lib, k, w):
    keys = random_keys(k)
    got = np.array([lib.shk_key_owner(k, w, x) for x in keys.tolist()], dtype=np.uint32)
    assert int(got.max()) < w
    assert np.array_equal(got, owners_py(k, w, keys))
    share = np.bincount(got, minlength=w) / N_KEYS
    assert share.min() >= 0.8 / w and share.max() <= 1.2 / w, (share.min() * w, share.max() * w)
    # the two ends of the key space and the narrow/wide multiplier boundary (k 21 | 22) are in the parametrisation;
    # bits above 2k in the argument do not matter (a canonical k-mer has none)
    assert lib.shk_key_owner(k, w, int(keys[0]) | (1 << 63)) == int(got[0])


@pytest.mark.parametrize("k,w", [(0, 2), (32, 2), (33, 8), (0xFFFFFFFF, 2), (21, 3), (21, 6), (21, 0), (21, 128), (21, 96), (15, 65)])
def test_refused_arguments(lib, k, w):
    assert lib.shk_key_owner(k, w, 12345) == NONE


def test_key_owner_driver_clean_under_asan_ubsan():
    """The function under a stand-alone caller (tests/native/key_owner_driver.cpp) with AddressSanitizer and UBSan:
    nothing is preloaded, the runtimes are linked statically."""
    import subprocess
    csrc = os.path.join(ROOT, "sharkmer_amd", "csrc")
    probe = subprocess.run(["g++", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not (os.path.isabs(probe) and os.path.exists(probe)):
        pytest.skip("no asan runtime in this toolchain")
    subprocess.check_call(["make", "-C", csrc, "key_owner_driver"], stdout=subprocess.DEVNULL)
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "halt_on_error=1:abort_on_error=0:detect_leaks=1"
    env["UBSAN_OPTIONS"] = "halt_on_error=1:print_stacktrace=1"
    r = subprocess.run([os.path.join(csrc, "key_owner_driver")], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert re.fullmatch(r"key_owner_driver ok: (\d+) calls\n", r.stdout), r.stdout
