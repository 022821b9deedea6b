"""lsx_set_option / lsx_get_option key by key: which keys can be set, read or both, the values a set accepts, the
nearest values it refuses, and the defaults of a fresh handle.  The expected table below is written out by hand from the
two if / else chains of api.hip; nothing here is read or generated from the library, so a key that drifts shows,
whatever form the two functions take later.  The test uses a handle of its own and launches no kernel.
"""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu

INT_MAX = 2 ** 31 - 1
ERR_ARG = -1

ON_OFF = ((0, 1), (-1, 2))
FROM_ZERO = ((0, INT_MAX), (-1,))

# key: (the smallest and largest accepted value or every value of a short list, the nearest refused values around them)
WRITABLE_ONLY = {
    "gemm_tiles32": ON_OFF,
    "gemm_queue_test": ((0, 3), (-1, 4)),
    "rref_blocked": ON_OFF,
    "xrows_limit": FROM_ZERO,
    "getri_structured": ON_OFF,
    "x_events": ON_OFF,
    "hybrid": ON_OFF,
    "prof_sample": ((1, INT_MAX), (0, -1)),
    "panel_spin_limit": ((-5, -1, 1, INT_MAX, -INT_MAX - 1), (0,)),
    "trsv_spin_limit": FROM_ZERO,
    "panel_debug": ((0, 1, 7, -3), ()),          # any value is accepted (and stored as 0 or 1)
}
READ_WRITE = {
    "nb": ((16, 128), (0, 8, 15, 17, 24, 127, 129, 144)),      # 16 .. 128 in multiples of 16
    "panel": ((0, 4, 3), (-1, 5)),                             # 1 and 2: test_panel_superseded
    "trsv": ((0, 2), (-1, 3)),
    "gemm_stagger": ((0, 64), (-1, 65)),
    "gemm_waves": ((0, 4, 8), (-1, 1, 2, 3, 5, 6, 7, 9)),
    "kblock": ((1, 2), (0, 3)),
    "panel_rt": ((2, 4, 8), (0, 1, 3, 5, 7, 9)),
    "panel_nt": ((0, 256, 512, 1024), (-1, 1, 255, 257, 511, 513, 1023, 1025)),
    "getri_pairs": ON_OFF,
    "left_per_step": ON_OFF,
    "chain_fused": ON_OFF,
    "rref_first_fast": ON_OFF,
    "chain_wait_limit": FROM_ZERO,
    "lookahead": ON_OFF,
    "lookahead_min": FROM_ZERO,
    "getrs_t_blocked_min": FROM_ZERO,
    "gesvdj_max_sweeps": ((1, 60), (0, 61)),
    "syevj_max_sweeps": ((1, 100), (0, 101)),
    "potrs_few_max": ((0, 8), (-1, 9)),
    "potri_order": ON_OFF,
    "lauum_descending": ON_OFF,
}
READABLE_ONLY = (
    "rref_first_used", "panel_fallbacks", "num_cu", "gecon_solves", "gerfs_steps", "gerfs_solves", "getrs_t_path",
    "potrs_path", "potri_tiles", "gesvdj_sweeps", "gesvdj_rotations", "syevj_sweeps", "syevj_rotations", "pocon_solves",
    "porfs_steps", "porfs_solves",
)
# the defaults common.h states
DEFAULTS = {"nb": 128, "panel": 4, "lookahead": 1, "trsv": 2, "gesvdj_max_sweeps": 30, "syevj_max_sweeps": 60,
            "potrs_few_max": 0, "getrs_t_blocked_min": 64}


class Options:
    """The two entry points on a handle of this module's own: (return code, last error) and (return code, value, last error)."""

    def __init__(self):
        from linalg_solver_amd import _native

        self.handle = _native.Handle()
        self.lib = self.handle.lib

    def set(self, key, value):
        rc = self.lib.lsx_set_option(self.handle.ptr, key.encode(), value)
        return rc, self.lib.lsx_last_error()

    def get(self, key):
        v = C.c_int(-12345)
        rc = self.lib.lsx_get_option(self.handle.ptr, key.encode(), C.byref(v))
        return rc, v.value, self.lib.lsx_last_error()


@pytest.fixture(scope="module")
def fresh():
    """A handle on which nothing has been set yet, destroyed at the end; test_defaults runs first and only reads."""
    o = Options()
    yield o
    o.handle.close()


@pytest.fixture
def opt():
    o = Options()
    yield o
    o.handle.close()


def test_table_is_the_whole_interface():
    assert len(WRITABLE_ONLY) == 11 and len(READ_WRITE) == 21 and len(READABLE_ONLY) == 16
    assert len(set(WRITABLE_ONLY) | set(READ_WRITE) | set(READABLE_ONLY)) == 48


def test_defaults(fresh):
    for key, want in DEFAULTS.items():
        assert fresh.get(key)[:2] == (0, want), key


@pytest.mark.parametrize("key", sorted(WRITABLE_ONLY) + sorted(READ_WRITE))
def test_accepted_and_refused_values(opt, key):
    accepted, refused = WRITABLE_ONLY[key] if key in WRITABLE_ONLY else READ_WRITE[key]
    for v in refused:
        rc, err = opt.set(key, v)
        assert rc == ERR_ARG and b"bad argument" in err, (key, v, rc, err)
    for v in accepted:
        rc, err = opt.set(key, v)
        assert rc == 0, (key, v, rc, err)
        if key in READ_WRITE:
            assert opt.get(key)[:2] == (0, v), (key, v)      # a set, then a get, returns the value set
            for w in refused:                                # and a refused set leaves it alone
                assert opt.set(key, w)[0] == ERR_ARG
                assert opt.get(key)[:2] == (0, v), (key, v, w)


@pytest.mark.parametrize("key", sorted(WRITABLE_ONLY))
def test_writable_only_keys_cannot_be_read(opt, key):
    rc, value, err = opt.get(key)
    assert rc == ERR_ARG and b"unknown option" in err and key.encode() in err, (key, rc, err)
    assert value == -12345                                   # nothing was written


@pytest.mark.parametrize("key", READABLE_ONLY)
def test_readable_only_keys_cannot_be_set(opt, key):
    rc, before, err = opt.get(key)
    assert rc == 0, (key, err)
    for v in (0, 1):
        rc, err = opt.set(key, v)
        assert rc == ERR_ARG and b"unknown option" in err and key.encode() in err, (key, v, rc, err)
    assert opt.get(key)[:2] == (0, before)


def test_counters_of_a_fresh_handle(fresh):
    for key in READABLE_ONLY:
        rc, value, err = fresh.get(key)
        assert rc == 0, (key, err)
        assert value == 0 or (key == "num_cu" and value > 0), (key, value)


def test_panel_superseded(opt):
    assert opt.get("panel")[:2] == (0, 4)
    for v in (1, 2):
        rc, err = opt.set("panel", v)
        assert rc == ERR_ARG and b"superseded" in err, (v, rc, err)
        assert opt.get("panel")[:2] == (0, 4)
    for v in (-1, 5):                                        # out of range altogether: the generic message
        rc, err = opt.set("panel", v)
        assert rc == ERR_ARG and b"bad argument" in err and b"superseded" not in err, (v, rc, err)


def test_special_values(opt):
    assert opt.set("panel_debug", 7)[0] == 0
    assert opt.set("prof_sample", 0)[0] == ERR_ARG and opt.set("prof_sample", 1)[0] == 0
    assert opt.set("panel_spin_limit", 0)[0] == ERR_ARG and opt.set("panel_spin_limit", -5)[0] == 0


def test_unknown_key(opt):
    for key in ("no_such_option", "", "NB", "nb ", "panel_mode"):
        rc, err = opt.set(key, 1)
        assert rc == ERR_ARG and b"unknown option" in err, (key, rc, err)
        rc, _, err = opt.get(key)
        assert rc == ERR_ARG and b"unknown option" in err, (key, rc, err)


def test_null_arguments(opt):
    lib, h = opt.lib, opt.handle.ptr
    v = C.c_int(0)
    assert lib.lsx_set_option(h, None, 1) == ERR_ARG and b"bad argument" in lib.lsx_last_error()
    assert lib.lsx_get_option(h, None, C.byref(v)) == ERR_ARG and b"bad argument" in lib.lsx_last_error()
    assert lib.lsx_get_option(h, b"nb", None) == ERR_ARG and b"bad argument" in lib.lsx_last_error()
    assert lib.lsx_set_option(None, b"nb", 64) == ERR_ARG and lib.lsx_get_option(None, b"nb", C.byref(v)) == ERR_ARG
