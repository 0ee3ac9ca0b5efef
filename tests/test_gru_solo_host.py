"""zs_gru_solo: which launches the plan gives to the one-workgroup GRU kernels (bf16, H = 128), for grids small enough to fit any
device (B <= 16).  The query runs the launches' own plan function; no GPU is touched."""
import pytest


@pytest.fixture(scope='module')
def lib():
    import zs_amd  # noqa: F401
    from zs_amd import _lib
    _lib.lib()
    return _lib


def test_gru_solo_query(lib):
    q, path = lib.lib().zs_gru_solo, lib.lib().zs_gru_path
    BF16, F32, WIDE = lib.ZS_BF16, lib.ZS_F32, lib.ZS_GRU_PATH_WIDE
    old = {k: lib.set_option(k, v) for k, v in (('gru_persist', 1), ('gru_wide', 1), ('gru_solo_max_h', 128), ('gru_spin_limit', 1 << 21))}
    try:
        for pas in (0, 1):
            for B, T in ((1, 2), (16, 3), (9, 16)):
                assert q(pas, BF16, B, T, 128, 1, 1) == 1
                assert path(pas, BF16, B, T, 128, 1, 1) == WIDE
            for H in (256, 512):                                   # W_hh does not fit one workgroup: the hand-off kernels
                assert q(pas, BF16, 16, 5, H, 1, 1) == 0 and path(pas, BF16, 16, 5, H, 1, 1) == WIDE
            assert q(pas, BF16, 16, 5, 128, 1, 0) == 0              # not WIDE: operands without the 16-byte layout,
            assert q(pas, F32, 16, 5, 128, 1, 1) == 0               # fp32,
            assert q(pas, BF16, 16, 1, 128, 1, 1) == 0              # T = 1,
            assert q(pas, BF16, 16, 5, 96, 1, 1) == 0 and q(pas, BF16, 16, 5, 72, 1, 1) == 0
            for knob, v in (('gru_solo_max_h', 0), ('gru_solo_max_h', 127), ('gru_spin_limit', 0), ('gru_wide', 0), ('gru_persist', 0)):
                before = path(pas, BF16, 16, 5, 128, 1, 1)
                prev = lib.set_option(knob, v)
                try:
                    assert q(pas, BF16, 16, 5, 128, 1, 1) == 0, (knob, v)
                    if knob in ('gru_solo_max_h', 'gru_spin_limit'):    # the variant is inside WIDE: zs_gru_path does not move
                        assert path(pas, BF16, 16, 5, 128, 1, 1) == before == WIDE
                finally:
                    lib.set_option(knob, prev)
            assert q(pas, BF16, 16, 5, 128, 1, 1) == 1
        assert q(0, BF16, 16, 5, 128, 0, 1) == 0                    # the forward needs W_hh gate-interleaved ...
        assert q(1, BF16, 16, 5, 128, 0, 1) == 1                    # ... the BPTT reads the transposed packing
        lib.set_option('gru_solo_max_h', -3)                        # stored as 0
        assert lib.get_option('gru_solo_max_h') == 0 and q(0, BF16, 16, 5, 128, 1, 1) == 0
        lib.set_option('gru_solo_max_h', 512)                       # stored as given; the kernels exist for H = 128 only
        assert lib.get_option('gru_solo_max_h') == 512
        assert q(0, BF16, 16, 5, 128, 1, 1) == 1 and q(0, BF16, 16, 5, 256, 1, 1) == 0
    finally:
        for k, v in old.items():
            lib.set_option(k, v)


def test_gru_solo_refuses_bad_arguments(lib):
    q = lib.lib().zs_gru_solo
    BF16 = lib.ZS_BF16
    for args in ((2, BF16, 4, 8, 128, 1, 1), (-1, BF16, 4, 8, 128, 1, 1), (0, 7, 4, 8, 128, 1, 1), (0, BF16, 0, 8, 128, 1, 1),
                 (0, BF16, 4, 0, 128, 1, 1), (0, BF16, 4, 8, 0, 1, 1), (0, BF16, 4, 8, 100, 1, 1)):
        assert q(*args) < 0, args
        assert 'zs_gru_solo' in lib.last_error()
