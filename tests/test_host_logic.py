"""CPU tests: the C ABI library loads and exports every declared symbol with the declared struct layouts,
the product path fails loudly without a GPU, and the host logic (hps, dataloader, segmenter, CLI, data-parallel
reducer over gloo) behaves like the reference's."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import zs_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lib():
    import zs_amd  # noqa: F401
    from zs_amd import _lib, build
    build.build(verbose=False)
    return _lib


def test_library_exports_every_declared_symbol(lib):
    L = lib.lib()
    assert len(lib.FUNCTIONS) >= 24
    missing = [f for f in lib.FUNCTIONS if not hasattr(L, f)]
    assert not missing, missing
    assert L.zs_abi_version() == lib.ENUMS['ZS_ABI_VERSION']


def test_struct_layouts_match_the_c_compiler(lib, tmp_path):
    names = list(lib.STRUCTS)
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){\n' % lib.HEADER
    for n in names:
        src += 'printf("%s %%zu\\n", sizeof(%s));\n' % (n, n)
        for f, _ in lib._STRUCT_FIELDS[n]:
            src += 'printf("%s.%s %%zu\\n", offsetof(%s,%s));\n' % (n, f, n, f)
    src += 'return 0;}\n'
    c = tmp_path / 'sz.c'
    c.write_text(src)
    subprocess.check_call(['gcc', str(c), '-o', str(tmp_path / 'sz')])
    for line in subprocess.check_output([str(tmp_path / 'sz')]).decode().split('\n'):
        if not line:
            continue
        k, v = line.split()
        if '.' in k:
            n, f = k.split('.')
            assert getattr(lib.STRUCTS[n], f).offset == int(v), k
        else:
            assert ctypes.sizeof(lib.STRUCTS[k]) == int(v), k


def _c_kind(ct):
    """'<size><p|f|i|u>' of a ctypes type: pointer (c_void_p and c_char_p alike), floating, signed, unsigned."""
    if ct in (ctypes.c_void_p, ctypes.c_char_p):
        k = 'p'
    elif ct in (ctypes.c_float, ctypes.c_double):
        k = 'f'
    else:
        k = 'i' if ct(-1).value < 0 else 'u'
    return '%d%s' % (ctypes.sizeof(ct), k)


def test_function_signatures_match_the_cxx_compiler(lib, tmp_path):
    """The function-side twin of the layout test: g++ prints the size and kind of the return type and of every parameter of each
    declared function; the restype / argtypes that lib() set on the loaded library must say the same, for every function."""
    src = ('#include <cstdio>\n#include <type_traits>\n#include "%s"\n'
           'template <class T> void one() {\n'
           '  std::printf(" %%zu%%c", sizeof(T), std::is_pointer<T>::value ? \'p\' : std::is_floating_point<T>::value ? \'f\' :\n'
           '              std::is_signed<T>::value ? \'i\' : \'u\');\n}\n'
           'template <class R, class... A> void show(const char* name, R (*)(A...)) {\n'
           '  std::printf("%%s", name); one<R>(); int order[] = {0, (one<A>(), 0)...}; (void)order; std::printf("\\n");\n}\n'
           'int main() {\n' % lib.HEADER)
    # (a null pointer of the function's type: the program reads declarations only and links against nothing)
    src += ''.join('  show("%s", (decltype(&%s))0);\n' % (f, f) for f in lib.FUNCTIONS) + '  return 0;\n}\n'
    c = tmp_path / 'sig.cpp'
    c.write_text(src)
    subprocess.check_call(['g++', '-std=c++11', str(c), '-o', str(tmp_path / 'sig')])
    L, seen = lib.lib(), []
    for line in subprocess.check_output([str(tmp_path / 'sig')]).decode().splitlines():
        name, ret = line.split()[:2]
        fn = getattr(L, name)
        assert fn.argtypes is not None, '%s: no argtypes declared' % name
        assert [_c_kind(fn.restype)] + [_c_kind(a) for a in fn.argtypes] == [ret] + line.split()[2:], line
        seen.append(name)
    assert seen == lib.FUNCTIONS and len(seen) >= 92


@pytest.mark.parametrize('proto, named', [
    ('short zs_bad(int32_t a);', 'zs_bad.*short'),                       # a return type with no mapping
    ('int zs_bad(int32_t a, long double b);', 'zs_bad.*long double'),    # a parameter type with no mapping
    ('unsigned long zs_bad(void);', "zs_bad.*'unsigned long'"),          # a type of several words is named whole
    ('int zs_bad(void (*cb)(int), void* stream);', 'zs_bad'),            # a declaration the prototype pattern cannot read
])
def test_header_parse_is_strict(lib, tmp_path, proto, named):
    hdr = open(lib.HEADER).read()
    same = tmp_path / 'same.h'
    same.write_text(hdr)
    parsed = lib.parse_header(str(same))
    assert parsed[1] == lib.FUNCTIONS == list(parsed[4]) and len(lib.FUNCTIONS) >= 92
    bad = tmp_path / 'bad.h'
    bad.write_text(hdr.replace('int zs_abi_version(void);', 'int zs_abi_version(void);\n' + proto))
    with pytest.raises(ValueError, match=named):
        lib.parse_header(str(bad))


def test_a_64_bit_address_survives_a_positional_entry_point(lib):
    """zs_gemm_conv_path reads the struct and dereferences none of its operands.  The struct's address goes in as a plain integer
    above 2^32, with no signature set by this test: the header's declaration alone must carry all 64 bits of it."""
    T, C = 128, 1024
    s = lib.STRUCTS['ZsGemmConv'](dtype=lib.ZS_BF16, A=0x10000, lda=C, a_batch_stride=T * C, B=256, T_in=T, T_out=T, taps=1, stride=1,
                                  pad_mode=lib.ZS_PAD_REFLECT, cin_pad=C, W=0x20000, ldw=C, N=C, n_pad=C, out=0x30000, ldc=C, out_cols=C,
                                  groups=1)
    addr = ctypes.addressof(s)
    assert type(addr) is int and addr >> 32, hex(addr)
    rc = lib.lib().zs_gemm_conv_path(addr)
    assert rc >= 0, lib.last_error()
    assert rc & 255 in (lib.ZS_GEMM_PATH_P8, lib.ZS_GEMM_PATH_RING_PP, lib.ZS_GEMM_PATH_RING, lib.ZS_GEMM_PATH_DMA64,
                        lib.ZS_GEMM_PATH_DMA128, lib.ZS_GEMM_PATH_REG) and rc >> 8 in (0, 1)
    s.n_pad = 192                                              # the same route gives an argument error as its ZS_E* code
    assert lib.lib().zs_gemm_conv_path(addr) == lib.ZS_EINVAL


def test_invalid_calls_return_errors_not_crashes(lib):
    with pytest.raises(lib.ZsError, match='null operand'):
        lib.call('zs_gemm_conv', 'ZsGemmConv', 0, dtype=0)
    with pytest.raises(lib.ZsError):
        lib.call('zs_instnorm_fwd', 'ZsInstNormFwd', 0, dtype=7)
    assert 'zs_' in lib.last_error()


def _knob_probes(key):
    """(value set, value stored) pairs for the normalisation documented at zs_set_option in zs_amd.h."""
    if key in ('gru_persist', 'gru_wide', 'norm_wide', 'gl_prefetch'):
        return [(2, 1), (-1, 1), (0, 0)]
    if key == 'gl_chains':
        return [(0, 1), (9, 4), (2, 2)]
    if key.startswith('norm_lim'):
        return [(5, 5), (0, 0)]          # stored as given (a negative value would come back as an error code)
    return [(-5, 0), (7, 7)]


def test_set_option_knobs_are_documented_and_normalised(lib):
    """Every knob defined in csrc/ is documented at zs_set_option with its environment variable and default; each stores the
    documented normalisation of what is set or read from the environment; an unknown key is an error.  No GPU is touched."""
    hdr = open(lib.HEADER).read()
    doc = hdr[hdr.index('/* Kernel-selection knobs'):hdr.index('int zs_set_option(')]
    documented = {k: (env, int(d)) for k, env, d in re.findall(r'^ \*   "(\w+)" \((ZS_\w+|-), (\d+)\):', doc, flags=re.M)}
    assert len(documented) == doc.count('\n *   "')
    csrc = os.path.join(ROOT, 'zerospeech-tts-without-t_amd', 'csrc')
    defined = []
    for f in sorted(os.listdir(csrc)):
        defined += re.findall(r'\b\w+\("(\w+)", (?:"(ZS_\w+)"|nullptr), ', open(os.path.join(csrc, f)).read())
    assert len(defined) == len({k for k, _ in defined}), defined
    assert {k: env or '-' for k, env in defined} == {k: env for k, (env, _) in documented.items()}
    for key in documented:
        orig = lib.set_option(key, 0)
        try:
            for value, stored in _knob_probes(key):
                lib.set_option(key, value)
                assert lib.set_option(key, value) == stored, (key, value)
        finally:
            lib.set_option(key, orig)
    with pytest.raises(lib.ZsError, match='unknown key no_such_knob'):
        lib.set_option('no_such_knob', 1)
    # defaults, and environment values normalised like set values, in a process of their own
    env = {k: v for k, v in os.environ.items() if k != 'ZS_OPTIONS' and k not in {e for e, _ in documented.values()}}
    env.update(ZS_GRU_PERSIST='2', ZS_GEMM_RING_MIN_TILES='-7')
    script = 'import json, sys, zs_amd; from zs_amd import _lib as L; print(json.dumps({k: L.set_option(k, 1) for k in sys.argv[1:]}))'
    out = subprocess.check_output([sys.executable, '-c', script] + list(documented), env=env, cwd=ROOT, timeout=300)
    want = {k: d for k, (_, d) in documented.items()}
    want.update(gru_persist=1, gemm_ring_min_tiles=0)
    assert json.loads(out.decode().strip().splitlines()[-1]) == want


def test_gru_path_query_cases_independent_of_the_cu_count(lib):
    """zs_gru_path: the plan of a zs_gru_fwd (pass 0) / zs_gru_bwd (pass 1) launch, for grids small enough to fit any device
    (B <= 16, H <= 512: at most 16 workgroups).  No GPU is touched."""
    q = lib.lib().zs_gru_path
    WIDE, PERSIST, FUSED, GEMM = (lib.ZS_GRU_PATH_WIDE, lib.ZS_GRU_PATH_PERSIST, lib.ZS_GRU_PATH_STEP_FUSED,
                                  lib.ZS_GRU_PATH_STEP_GEMM)
    F32, BF16 = lib.ZS_F32, lib.ZS_BF16

    def path(pas, dt, T, H, inter=1, aligned=1, B=16):
        rc = q(pas, dt, B, T, H, inter, aligned)
        assert rc >= 0, lib.last_error()
        return rc & 255, rc >> 8

    old = {k: lib.set_option(k, 1) for k in ('gru_persist', 'gru_wide')}
    try:
        for pas in (0, 1):
            for dt in (F32, BF16):
                for H in (8, 40, 72, 520):                       # H % 32 != 0: a product launch and a gate launch per step
                    assert path(pas, dt, 9, H) == (GEMM, 0)
                for T in (2, 9):
                    assert path(pas, dt, T, 96) == (FUSED, 0)   # no persistent kernel for H = 96
                for H in (64, 128, 256, 512):                  # T = 1: nothing to persist
                    assert path(pas, dt, 1, H) == (FUSED, 0)
            # bf16, H in {128, 256, 512}: the wide tiling when the operands allow 16-byte transfers, else the 32 x 32 / 16 x 64 one
            for H, per, perb in ((128, 1, 3), (256, 2, 6), (512, 4, 12)):
                assert path(pas, BF16, 2, H) == (WIDE, 0)
                assert path(pas, BF16, 2, H, aligned=0) == (PERSIST, per if pas == 0 else perb)
        assert path(0, BF16, 9, 128, inter=0) == (GEMM, 0)       # the forward's fused paths need W_hh gate-interleaved ...
        assert path(1, BF16, 9, 128, inter=0) == (WIDE, 0)       # ... the BPTT reads the transposed packing
        for H, per, perb in ((64, 1, 3), (128, 2, 6), (256, 4, 12)):   # fp32 never takes the wide kernels
            assert path(0, F32, 5, H) == (PERSIST, per) and path(1, F32, 5, H) == (PERSIST, perb)
        for pas in (0, 1):
            assert path(pas, F32, 5, 512)[0] == FUSED                    # fp32 H = 512: no register-resident W_hh slice
            assert path(pas, BF16, 5, 192)[0] == FUSED                   # PER / PERB of 1.5 / 4.5
        lib.set_option('gru_wide', 0)
        for pas in (0, 1):
            assert path(pas, BF16, 2, 512) == (PERSIST, 4 if pas == 0 else 12)
        lib.set_option('gru_persist', 0)
        for pas in (0, 1):
            for dt in (F32, BF16):
                assert path(pas, dt, 9, 128) == (FUSED, 0)
                assert path(pas, dt, 9, 72) == (GEMM, 0)
        lib.set_option('gru_wide', 1)
        assert path(0, BF16, 9, 512) == (FUSED, 0)                       # gru_wide alone does not make a launch persistent
    finally:
        for k, v in old.items():
            lib.set_option(k, v)
    assert q(2, BF16, 4, 8, 128, 1, 1) < 0 and 'zs_gru_path' in lib.last_error()
    assert q(0, 7, 4, 8, 128, 1, 1) < 0
    assert q(0, BF16, 4, 8, 100, 1, 1) < 0                               # H % 8 != 0 is refused by the launches too


def test_gemm_conv_path_query(lib):
    """zs_gemm_conv_path: the kernel a zs_gemm_conv launch would take (the launch's own plan function), under the default knobs at
    the production shapes and with every dispatch knob flipped.  Operands are dummy aligned non-null integers: the query
    dereferences nothing and touches no GPU."""
    q = lib.lib().zs_gemm_conv_path
    P8, RPP, RING, D64, D128, REG = (lib.ZS_GEMM_PATH_P8, lib.ZS_GEMM_PATH_RING_PP, lib.ZS_GEMM_PATH_RING, lib.ZS_GEMM_PATH_DMA64,
                                     lib.ZS_GEMM_PATH_DMA128, lib.ZS_GEMM_PATH_REG)
    PTR = 0x10000

    def rup(x, m):
        return (x + m - 1) // m * m

    def path(B=256, T=128, N=1024, Cin=1024, k=1, dtype=lib.ZS_BF16, **kw):
        kc = 64 if dtype == lib.ZS_BF16 else 32
        cin_pad = rup(Cin, kc)
        a = dict(dtype=dtype, A=PTR, lda=cin_pad, a_batch_stride=T * cin_pad, B=B, T_in=T, T_out=T, taps=k, stride=1, pad_left=k // 2,
                 pad_mode=lib.ZS_PAD_REFLECT, gather=0, cin_pad=cin_pad, W=2 * PTR, ldw=k * cin_pad, N=N, n_pad=rup(N, 128), out=3 * PTR,
                 ldc=rup(N, 32), out_cols=rup(N, 32), groups=1)
        a.update(kw)
        s = lib.STRUCTS['ZsGemmConv'](**a)
        rc = q(ctypes.addressof(s))
        assert rc >= 0, lib.last_error()
        return rc & 255, rc >> 8

    keys = ('gemm_dma', 'gemm_ring', 'gemm_ring_min_tiles', 'gemm_pp', 'gemm_p8', 'gemm_p8_min_tiles', 'gemm_dma64',
            'gemm_dma64_max_tiles')
    defaults = (1, 1, 256, 1, 1, 200, 1, 256)
    old = {k: lib.set_option(k, v) for k, v in zip(keys, defaults)}
    try:
        # the bench size under the default knobs: B = 256, seg_len = 128
        assert path(N=128, Cin=513, k=7) == (D128, 0)            # conv bank: 256 tiles of 128 x 128, one tile column
        assert path(N=513) == (RPP, 0)                           # final linear: n_pad 640, 128 * 5 ring tiles
        assert path(N=1024) == (P8, 1)                           # plain bf16 row output: register epilogue
        assert path(N=1024, dtype=lib.ZS_F32) == (P8, 0)         # fp32 never takes it
        assert path(N=1024, out_f32=1) == (P8, 0)
        assert path(N=1024, out_cols=516, ldc=1056) == (P8, 0)
        assert path(N=1024, pre_vec=4 * PTR, pre_vec_ld=1024, vec_idx=5 * PTR, T=24, B=2048) == (P8, 0)
        assert path(N=1024, pre_vec=4 * PTR, pre_vec_ld=1024, vec_idx=5 * PTR, T=16, B=2048) == (P8, 1)
        assert path(N=1024, out=3 * PTR + 8) == (P8, 0)          # rows not 16-byte aligned
        assert path(N=1024, add_src=4 * PTR, add_ld=1024, add_f32=1) == (P8, 0)
        assert path(N=1024, add_src=4 * PTR, add_ld=1024) == (P8, 1)
        assert path(N=1024, act=lib.ZS_ACT_TANH) == (P8, 0)
        assert path(N=2048, store_mode=lib.ZS_STORE_SPLIT2, out_cols=1024, ldc=1024, k=3) == (P8, 1)
        assert path(B=1, T=129, N=1024, k=3) == (D64, 0)         # batch-1 inference: 16 tiles of 128 x 128
        # n_pad = 384 is never P8, whatever the tile count
        assert path(N=384, B=2048)[0] == RPP
        lib.set_option('gemm_p8_min_tiles', 0)
        assert path(N=384, B=1, T=64)[0] != P8 and path(N=260, B=1, T=64)[0] != P8
        assert path(N=260, n_pad=512, B=1, T=64)[0] == P8
        lib.set_option('gemm_p8_min_tiles', 200)
        # the tile-count thresholds, from both sides
        assert path(B=100, T=128, N=1024)[0] == P8               # 50 * 4 = 200 tiles of 256 x 256
        assert path(B=99, T=128, N=1024)[0] == P8                # 12672 rows: still 50 row tiles
        assert path(B=98, T=128, N=1024)[0] == RPP               # 49 * 4 = 196 < 200; 49 * 8 = 392 ring tiles
        lib.set_option('gemm_p8_min_tiles', 201)
        assert path(B=100, T=128, N=1024)[0] == RPP
        lib.set_option('gemm_p8_min_tiles', 200)
        lib.set_option('gemm_p8', 0)
        assert path(N=1024) == (RPP, 0)
        lib.set_option('gemm_pp', 0)
        assert path(N=1024) == (RING, 0) and path(N=513) == (RING, 0)
        lib.set_option('gemm_pp', 1)
        assert path(B=64, T=128, N=1024)[0] == RPP               # 32 * 8 = 256 ring tiles
        assert path(B=63, T=128, N=1024)[0] == RPP               # 8064 rows: still 32 row tiles
        assert path(B=62, T=128, N=1024)[0] == D128              # 31 * 8 = 248 < 256; 62 * 8 128-row tiles: too many for DMA64
        lib.set_option('gemm_ring_min_tiles', 248)
        assert path(B=62, T=128, N=1024)[0] == RPP
        lib.set_option('gemm_ring_min_tiles', 256)
        lib.set_option('gemm_ring', 0)
        assert path(N=1024) == (D128, 0) and path(N=513) == (D128, 0)
        # 64-row tiles: twice the 128 x 128 tile count at most gemm_dma64_max_tiles
        assert path(B=16, T=128, N=1024)[0] == D64               # 16 * 8 = 128 tiles
        assert path(B=17, T=128, N=1024)[0] == D128              # 136 tiles
        lib.set_option('gemm_dma64_max_tiles', 272)
        assert path(B=17, T=128, N=1024)[0] == D64
        lib.set_option('gemm_dma64_max_tiles', 256)
        lib.set_option('gemm_dma64', 0)
        assert path(B=16, T=128, N=1024)[0] == D128 and path(B=1, T=129, N=1024, k=3)[0] == D128
        lib.set_option('gemm_dma64', 1)
        # a colsum launch whose samples do not fit 64-row tiles is never DMA64
        cs = dict(colsum=6 * PTR, colsum_ld=1024, gather=1, pad_left=0, pad_mode=lib.ZS_PAD_ZERO)
        assert path(B=4, T=128, N=256, **cs)[0] == D128 and path(B=8, T=64, N=256, **cs)[0] == D64
        assert path(B=32, T=16, N=256, **cs)[0] == D64
        lib.set_option('gemm_ring', 1)
        lib.set_option('gemm_dma', 0)                            # the register-staged kernel, whatever the other knobs say
        for kw in (dict(N=1024), dict(N=513), dict(N=128, Cin=513, k=7), dict(B=1, T=129, N=1024, k=3)):
            assert path(**kw) == (REG, 0)
            assert path(dtype=lib.ZS_F32, **kw) == (REG, 0)
        lib.set_option('gemm_dma', 1)
        lib.set_option('gemm_p8', 1)
        assert path(N=1024) == (P8, 1)
    finally:
        for k, v in old.items():
            lib.set_option(k, v)

    def bad(**kw):
        a = dict(dtype=lib.ZS_BF16, A=PTR, lda=64, a_batch_stride=64 * 16, B=2, T_in=16, T_out=16, taps=1, stride=1, cin_pad=64,
                 W=2 * PTR, ldw=64, N=64, n_pad=128, out=3 * PTR, ldc=64, out_cols=64)
        a.update(kw)
        s = lib.STRUCTS['ZsGemmConv'](**a)
        rc = q(ctypes.addressof(s))
        return rc < 0 and 'zs_gemm_conv' in lib.last_error()

    assert not bad()
    assert q(None) < 0 and 'zs_gemm_conv' in lib.last_error()
    assert bad(A=0) and bad(W=0) and bad(out=0) and bad(dtype=7) and bad(cin_pad=48) and bad(ldw=32) and bad(n_pad=64)
    assert bad(n_pad=192) and bad(A=PTR + 2) and bad(B=0) and bad(N=0)
    assert bad(N=63, store_mode=lib.ZS_STORE_SPLIT2) and bad(pre_vec=4 * PTR) and bad(colsum=4 * PTR, T_out=24, T_in=24)
    assert bad(lengths=4 * PTR, gather=1)
    # reflect padding as long as the sample is refused with torch's message; one row shorter is accepted
    assert bad(taps=7, pad_left=3, pad_mode=lib.ZS_PAD_REFLECT, T_in=3, T_out=3, ldw=7 * 64)
    assert 'Padding size should be less than the corresponding input dimension' in lib.last_error()
    assert not bad(taps=7, pad_left=3, pad_mode=lib.ZS_PAD_REFLECT, T_in=4, T_out=4, ldw=7 * 64)


class _WgradQuery(object):
    """zs_gemm_wgrad_path on structs with dummy aligned non-null operands (nothing is dereferenced, no GPU is touched), and the
    split-K rule of the plan restated."""

    def __init__(self, lib):
        self.lib, self.L = lib, lib.lib()
        self.P8, self.DMA, self.REG = lib.ZS_WGRAD_PATH_P8, lib.ZS_WGRAD_PATH_DMA, lib.ZS_WGRAD_PATH_REG
        self.PTR = 0x10000

    @staticmethod
    def rup(x, m):
        return (x + m - 1) // m * m

    def struct(self, B=64, T=128, Cout=1024, Cin=1024, k=1, dtype=None, conv=True, **kw):
        lib, rup, PTR = self.lib, self.rup, self.PTR
        dtype = lib.ZS_BF16 if dtype is None else dtype
        es = 2 if dtype == lib.ZS_BF16 else 4
        a = dict(dtype=dtype, dY=PTR, ldy=rup(Cout, 32), y_cols=rup(Cout, 16 // es), X=2 * PTR, ldx=rup(Cin, 32), x_batch_stride=T * rup(Cin, 32),
                 x_cols=rup(Cin, 16 // es), B=B, T_in=T, T_out=T, taps=k, stride=1, pad_left=k // 2, pad_mode=lib.ZS_PAD_REFLECT, Cout=Cout,
                 Cin=Cin, dW=3 * PTR, so=Cin * k, si=k if conv else 1, sj=1 if conv else Cin, workspace=4 * PTR)
        a.update(kw)
        return lib.STRUCTS['ZsGemmWgrad'](**a)

    def path(self, **kw):
        """(kernel, reduce, splits, rows per split); the workspace size and the rounding of rows per split follow the reported plan."""
        rup = self.rup
        s = self.struct(**kw)
        k, r, sp, rps = self.lib.wgrad_path(s)
        tile = 256 if k == self.P8 else 128
        need = sp * (rup(s.Cout, tile) * s.taps * rup(s.Cin, tile) + rup(s.Cout, tile)) * 4
        assert self.L.zs_gemm_wgrad_workspace_bytes(ctypes.byref(s)) == need, kw
        assert rps % (64 if k == self.P8 else 32) == 0 and rps == rup(-(-s.B * s.T_out // sp), 64 if k == self.P8 else 32), kw
        return k, r, sp, rps

    @staticmethod
    def plan128(M, tiles, target=448):
        return max(1, min(-(-target // tiles), -(-M // 256), 1024))

    @staticmethod
    def plan256(M, tiles, wgs=256, slab=13):
        kt, best, bs = -(-M // 64), 1e30, 1
        for sp in range(1, 65):
            if sp * 4 > kt:
                break
            cost = -(-tiles * sp // wgs) * (-(-kt // sp) + slab)
            if cost < best - 1e-9:
                best, bs = cost, sp
        return bs


@pytest.fixture
def wgrad_query(lib):
    """A _WgradQuery under the documented defaults of every weight-gradient knob; the knobs are restored afterwards."""
    keys = ('wgrad_p8', 'wgrad_dma', 'wgrad_reduce_taps', 'wgrad_alone', 'wgrad_p8_waste', 'wgrad_wgs', 'wgrad_wgs128', 'wgrad_slab_cost',
            'wgrad_wgs128_alone', 'wgrad_slab_cost_alone')
    defaults = (1, 1, 1, 0, 135, 256, 448, 13, 448, 13)
    old = {k: lib.set_option(k, v) for k, v in zip(keys, defaults)}
    try:
        yield _WgradQuery(lib)
    finally:
        for k, v in old.items():
            lib.set_option(k, v)


def test_gemm_wgrad_path_dispatch(lib, wgrad_query):
    """zs_gemm_wgrad_path (the launch's own plan function): the K-loop kernel under wgrad_p8 0 / 1 / 2, wgrad_dma and wgrad_p8_waste,
    both P8 thresholds from both sides, fp32 never P8 or DMA; the taps-reduce condition under wgrad_reduce_taps."""
    q = wgrad_query
    path, P8, DMA, REG, F32, BF16 = q.path, q.P8, q.DMA, q.REG, lib.ZS_F32, lib.ZS_BF16
    # the P8 rule: bf16, M >= 2048, (256 x 256 tiles x taps) * M >= 16 * 8192, padding waste at most wgrad_p8_waste / 100
    assert path()[:2] == (P8, 0)                                             # M 8192, 16 tiles
    assert path(B=1, T=8191)[0] == DMA and path(B=1, T=8192)[0] == P8        # t256 * M from both sides
    assert path(B=1, T=2047, Cout=2048, Cin=2048, k=3)[0] == DMA             # M from both sides (192 tiles)
    assert path(B=1, T=2048, Cout=2048, Cin=2048, k=3)[:2] == (P8, 1)
    assert path(dtype=F32)[0] == REG and path(B=1, T=2048, Cout=2048, Cin=2048, k=3, dtype=F32)[:2] == (REG, 1)
    big = dict(B=1024, T=128)                                                # M 131072: one tile is enough
    assert path(Cout=200, Cin=256, **big)[0] == P8                           # waste 1.28
    assert path(Cout=180, Cin=256, **big)[0] == DMA                          # waste 1.42
    lib.set_option('wgrad_p8_waste', 143)
    assert path(Cout=180, Cin=256, **big)[0] == P8
    lib.set_option('wgrad_p8_waste', 135)
    lib.set_option('wgrad_p8', 0)
    assert path()[0] == DMA and path(dtype=F32)[0] == REG
    lib.set_option('wgrad_dma', 0)
    assert path()[0] == REG and path(Cout=8, Cin=8, B=1, T=21)[0] == REG
    lib.set_option('wgrad_p8', 2)                                            # forced: any bf16 shape, never fp32
    assert path(Cout=8, Cin=8, B=1, T=21)[0] == P8 and path(Cout=180, Cin=256)[0] == P8
    assert path(Cout=8, Cin=8, B=1, T=21, dtype=F32)[0] == REG and path(dtype=F32)[0] == REG
    lib.set_option('wgrad_dma', 1)
    assert path(dtype=F32)[0] == REG                                         # fp32 never takes the LDS-DMA kernel either
    lib.set_option('wgrad_p8', 0)
    assert path(Cout=8, Cin=8, B=1, T=21, dtype=F32)[0] == REG and path(Cout=8, Cin=8, B=1, T=21)[0] == DMA
    # the taps reduce: a Conv1d weight (si == taps, sj == 1) with 1 < taps <= 256, whatever so
    for dt in (BF16, F32):
        assert path(k=3, dtype=dt)[1] == 1 and path(k=1, dtype=dt)[1] == 0
        assert path(k=3, dtype=dt, so=3 * 1024 + 40)[1] == 1
        assert path(k=3, dtype=dt, conv=False)[1] == 0                       # [co][tap][ci]: si 1, sj Cin
        assert path(k=3, dtype=dt, si=4)[1] == 0 and path(k=3, dtype=dt, sj=0)[1] == 0
        assert path(k=256, Cout=8, Cin=8, B=1, T=300, dtype=dt)[1] == 1 and path(k=257, Cout=8, Cin=8, B=1, T=300, dtype=dt)[1] == 0
    lib.set_option('wgrad_reduce_taps', 0)
    assert path(k=3)[1] == 0
    lib.set_option('wgrad_reduce_taps', 1)


def test_gemm_wgrad_path_splits(lib, wgrad_query):
    """Explicit splits with rows per split rounded to 32 (64 for P8), and splits = 0 against the split-K rule restated in
    _WgradQuery, under wgrad_alone and the workgroup / slab-cost knobs; the workspace size agrees with every reported plan."""
    q = wgrad_query
    path, plan128, plan256, P8, F32 = q.path, q.plan128, q.plan256, q.P8, lib.ZS_F32
    # explicit splits: rows per split rounded up to 32 (64 for P8), also where trailing splits get no rows
    assert path(B=1, T=200, splits=3)[2:] == (3, 96) and path(B=1, T=21, splits=5)[2:] == (5, 32)
    assert path(B=1, T=640, splits=7, dtype=F32)[2:] == (7, 96)
    lib.set_option('wgrad_p8', 2)
    assert path(B=1, T=200, splits=3)[2:] == (3, 128) and path(B=1, T=21, splits=5)[2:] == (5, 64)
    assert path(B=1, T=640, splits=7)[2:] == (7, 128)                        # splits 5 and 6 start at rows 640 and 768: empty
    # splits = 0: the plan's choice, restated above
    lib.set_option('wgrad_p8', 1)
    for alone in (0, 1):
        lib.set_option('wgrad_alone', alone)
        assert path(Cout=128, Cin=513, k=5)[2:] == (18, 480)                 # 25 tiles of 128 x 128: ceil(448 / 25)
        assert path(Cout=128, Cin=513, k=5, B=1, T=700)[2] == 3              # at most one split per 256 rows
        assert path(Cout=64, Cin=25, B=1 << 14, T=128, dtype=F32, conv=False)[2] == 448
        assert path(B=256, Cout=1024, Cin=1024)[2] == plan256(256 * 128, 16) and path(B=256)[0] == P8
        assert path(B=256, Cout=2048, Cin=1024, k=3)[2] == plan256(256 * 128, 96)
    lib.set_option('wgrad_wgs128_alone', 768)
    lib.set_option('wgrad_slab_cost_alone', 40)
    lib.set_option('wgrad_wgs', 128)
    for alone in (0, 1):
        lib.set_option('wgrad_alone', alone)
        assert path(Cout=128, Cin=513, k=5)[2] == plan128(8192, 25, 768 if alone else 448) == (31 if alone else 18)
        assert path(B=256)[2] == plan256(256 * 128, 16, wgs=128, slab=40 if alone else 13)
    lib.set_option('wgrad_wgs128', 0)                                        # 0: the built-in target
    lib.set_option('wgrad_alone', 0)
    assert path(Cout=128, Cin=513, k=5)[2] == 18


def test_gemm_wgrad_path_errors(lib, wgrad_query):
    """Every argument error comes back from zs_gemm_wgrad_path as the code and the text the launch itself gives (the launch
    returns before any GPU call); the workspace size is the launch's check alone."""
    q = wgrad_query
    L, struct, PTR, F32 = q.L, q.struct, q.PTR, lib.ZS_F32
    # every argument error: the code and the text of the launch itself
    launch = L.zs_gemm_wgrad

    def bad(text, **kw):
        small = dict(B=2, T=16, Cout=64, Cin=64)
        small.update(kw)
        s = struct(**small)
        rc = L.zs_gemm_wgrad_path(ctypes.addressof(s), None, None)
        e1 = lib.last_error()
        if rc >= 0:
            return False
        assert launch(ctypes.addressof(s), None) == rc == lib.ZS_EINVAL and lib.last_error() == e1 and text in e1, (kw, rc, e1)
        return True

    assert not bad('')
    assert L.zs_gemm_wgrad_path(None, None, None) == lib.ZS_EINVAL and launch(None, None) == lib.ZS_EINVAL
    for f in ('dY', 'X', 'dW', 'workspace'):
        assert bad('null operand', **{f: 0})
    assert bad('workspace must be 16-byte aligned', workspace=4 * PTR + 8)
    assert bad('bad dtype', dtype=7)
    for f in ('B', 'T_in', 'T_out', 'Cout', 'Cin', 'taps', 'stride'):
        assert bad('bad sizes', **{f: 0}), f
    for kw in (dict(dY=PTR + 2), dict(X=2 * PTR + 8), dict(ldy=68), dict(ldx=68), dict(x_batch_stride=16 * 64 + 4), dict(y_cols=60, Cout=60),
               dict(x_cols=60, Cin=60), dict(dtype=F32, ldy=66), dict(dtype=F32, x_cols=62, Cin=60)):
        assert bad('16-byte aligned', **kw), kw
    assert not bad('', dtype=F32, ldy=68, x_cols=60, Cin=60)                     # fp32: multiples of 4 elements
    for kw in (dict(y_cols=72), dict(x_cols=72), dict(y_cols=56), dict(x_cols=56), dict(Cout=65, y_cols=64, ldy=64), dict(Cin=65, x_cols=64, ldx=64)):
        assert bad('column bounds', **kw), kw
    assert bad('SPLIT2 needs even Cout', Cout=63, y_cols=64, co_split2=1) and not bad('', Cout=62, y_cols=64, co_split2=1)
    g2 = dict(T=24, k=9, w_in=6, w_out=6, taps_h=3)
    assert not bad('', **g2)
    for kw in (dict(w_in=-1), dict(w_out=0), dict(taps_h=0), dict(taps_h=2), dict(w_in=5), dict(w_out=5)):
        assert bad('2-D geometry', **dict(g2, **kw)), kw
    # the report does not look at the workspace size; the launch does, after the plan
    s = struct(B=2, T=16, Cout=64, Cin=64, workspace_bytes=16)
    assert L.zs_gemm_wgrad_path(ctypes.addressof(s), None, None) >= 0
    assert launch(ctypes.addressof(s), None) == lib.ZS_EWORKSPACE and 'workspace 16 <' in lib.last_error()


def test_no_cpu_fallback():
    import zs_amd  # noqa: F401
    from zs_amd import _lib
    from zs_amd.layers import Ctx
    from zs_amd.model import Encoder
    if torch.cuda.is_available():
        pytest.skip('has GPU')
    with pytest.raises(_lib.ZsError, match='no CPU'):
        Ctx('cpu')
    enc = Encoder(c_in=80, c_h1=16, c_h2=32, c_h3=16, enc_size=8, seg_len=128, enc_mode='multilabel_binary')
    with pytest.raises(_lib.ZsError, match='no CPU fallback'):
        enc(torch.rand(1, 80, 16))
    with pytest.raises(NotImplementedError):
        Encoder(enc_mode='nonsense')
    src = open(os.path.join(ROOT, 'zerospeech-tts-without-t_amd', 'model.py')).read() + \
        open(os.path.join(ROOT, 'zerospeech-tts-without-t_amd', 'engine.py')).read() + \
        open(os.path.join(ROOT, 'zerospeech-tts-without-t_amd', 'trainer.py')).read() + \
        open(os.path.join(ROOT, 'zerospeech-tts-without-t_amd', 'convert.py')).read()
    assert 'zs_oracle' not in src and 'oracle' not in src.replace('oracle/', '')      # product never imports the oracle


def test_hps_surface():
    from zs_amd.hps import HPS_KEYS, Hps, hp
    assert len(HPS_KEYS) == 32
    h = Hps(os.path.join(ROOT, 'hps', 'zerospeech_english.json')).get_tuple()
    assert (h.seg_len, h.enc_size, h.emb_size, h.n_speakers, h.batch_size, h.lr, h.max_grad_norm) == (128, 6, 1024, 102, 16, 1e-4, 5)
    assert (hp.sr, hp.n_fft, hp.hop_length, hp.win_length, hp.n_iter, hp.preemphasis, hp.max_db, hp.ref_db) == \
        (16000, 1024, 200, 800, 300, .97, 100, 20)
    d = dict(h._asdict())
    d.pop('lr')
    p = os.path.join(ROOT, 'tests', '_tmp_hps.json')
    try:
        json.dump(d, open(p, 'w'))
        with pytest.raises(TypeError):
            Hps(p)
        d['lr'] = 1e-4; d['extra'] = 1
        json.dump(d, open(p, 'w'))
        with pytest.raises(TypeError):
            Hps(p)
    finally:
        os.remove(p)


def test_dataloader_contract():
    from zs_amd.dataloader import DataLoader, SyntheticDataset
    ds = SyntheticDataset(40, seg_len=16, n_bins=513, n_speakers=7, seed=1)
    dl = DataLoader(ds, batch_size=16)
    c, x = next(dl)
    assert c.dtype == torch.int64 and c.shape == (16,) and x.dtype == torch.float32 and x.shape == (16, 16, 513)
    assert x.min() >= 1e-8 and x.max() <= 1.0
    assert dl.index == 16
    next(dl)                       # index 16 + 2*16 >= 40 -> wraps to 0 (dataloader.py:48-49)
    assert dl.index == 0
    c2, x2 = next(dl)
    assert torch.equal(c, c2) and torch.equal(x, x2)
    dl16 = DataLoader(SyntheticDataset(16, seg_len=8), batch_size=16)   # BASELINE config 1: one batch re-served forever
    a = next(dl16); b = next(dl16)
    assert torch.equal(a[1], b[1]) and dl16.index == 0


def test_segmenter_matches_oracle_and_text_format(tmp_path):
    from zs_amd import convert
    for n in (9, 100, 128, 129, 255, 256, 257, 300, 383, 384, 385, 700, 1000):
        if n <= 128:
            continue
        assert convert.fragments(n, 128) == O.fragment_plan(n, 128)[1], n
    with pytest.raises(RuntimeError, match='too short'):
        convert.fragments(129, 200)                      # one piece of 128 frames < seg_len 200 at idx 0
    enc = np.array([[1., 0., 1., 1.], [0., 0., 0., 1.]])
    convert.write_encodings(str(tmp_path / 'e.txt'), enc)
    assert open(str(tmp_path / 'e.txt')).read() == '1 0 1 1\n0 0 0 1\n' == O.encodings_text(enc)
    assert convert.parse_encodings(enc) == ['1 0 1 1', '0 0 0 1']
    rng = np.random.RandomState(0)
    y = np.concatenate([np.zeros(3000), rng.randn(8000) * 0.1, np.zeros(5000)])
    a, ia = convert.trim(y)
    b, ib = O.trim(y)
    assert ia == ib and np.array_equal(a, b) and 0 < len(a) < len(y)
    convert.write_wav(str(tmp_path / 'w.wav'), np.array([0.0, 0.5, -0.5, 1.0], dtype=np.float32), 16000)
    import wave
    with wave.open(str(tmp_path / 'w.wav')) as f:
        assert (f.getframerate(), f.getsampwidth(), f.getnchannels(), f.getnframes()) == (16000, 2, 1, 4)


def test_cli_surface(capsys):
    sys.path.insert(0, ROOT)
    import main
    args, hps = main.argument_runner(['--train_ae', '--hps_path', os.path.join(ROOT, 'hps', 'zerospeech_english_1024.json')])
    assert args.train_ae and args.g_mode == 'targeted_residual' and args.enc_mode == 'multilabel_binary' and hps.enc_size == 1024
    args, _ = main.argument_runner(['--test', '--enc_only', '--dataset', 'surprise', '--hps_path',
                                    os.path.join(ROOT, 'hps', 'zerospeech_surprise.json')])
    assert args.ckpt_dir == './ckpt_surprise' and args.dataset_path == './data/dataset_surprise.hdf5' and \
        args.synthesis_list == './data/surprise/synthesis.txt' and args.sub_result_dir == './surprise/'
    with pytest.raises(NotImplementedError):
        main.main(['--train_al', '--hps_path', os.path.join(ROOT, 'hps', 'zerospeech_english.json')])


def _dp_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'oracle'))
    import zs_amd  # noqa: F401
    from zs_amd import parallel
    from conftest import load_golden, sub_sd
    torch.set_num_threads(1)
    parallel.init_from_env('gloo')
    d, m = load_golden('train_f80.npz')
    g = torch.Generator().manual_seed(0)
    B = 4
    x = torch.rand(B, m['c_in'], 32, generator=g)
    c = torch.randint(0, m['n_spk'], (B,), generator=g)
    G = O.gumbel_from_uniform(torch.rand(B, 4, m['enc_size'], 2, generator=g))
    hp = dict(ns=m['ns'], enc_dp=0.0, enc_size=m['enc_size'], seg_len=m['seg_len'])
    lo, hi = parallel.shard_range(B, rank, world)
    _, (ge, gd), _, _ = O.train_ae_grads(sub_sd(d, 'enc0.'), sub_sd(d, 'dec0.'), x[lo:hi], c[lo:hi], hp, G=G[lo:hi])
    flat = torch.cat([v.reshape(-1) for v in list(ge.values()) + list(gd.values())])
    red = parallel.GradReducer(bucket_bytes=64 << 10)          # several buckets
    # tagged ranges in backward order (trainer.AEStep.plan): the decoder's ranges first, the encoder's last; a wait
    # for one tag leaves the other tag's collectives pending
    ne = sum(v.numel() for v in ge.values())
    cut = ne + (flat.numel() - ne) // 3
    red.start(flat[cut:], tag='dec')
    red.start(flat[ne:cut], tag='dec')
    red.start(flat[:ne], tag='enc')
    red.finish('dec')
    assert red.pending and all(t == 'enc' for t, _, _, _ in red.pending)
    red.finish('enc')
    assert not red.pending
    assert red.scale == 0.5
    flat = flat * red.scale            # the buffers hold the SUM over ranks; the consumer (zs_adam_clip) folds 1/world in
    if rank == 0:
        _, (fe, fd), _, _ = O.train_ae_grads(sub_sd(d, 'enc0.'), sub_sd(d, 'dec0.'), x, c, hp, G=G)
        full = torch.cat([v.reshape(-1) for v in list(fe.values()) + list(fd.values())])
        q.put(((flat - full).abs().max().item(), full.abs().max().item(), parallel.world_size()))
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def test_data_parallel_gradient_average_gloo():
    """world_size 2 over gloo: the averaged per-rank gradients equal the single-process global-batch gradient
    (segments are independent: InstanceNorm is per sample)."""
    import torch.multiprocessing as mp
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = 29500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    err, scale, world = q.get(timeout=240)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert world == 2 and err <= 2e-5 * scale, (err, scale)


def test_gradient_buckets_partition_the_flat_buffers_in_backward_order():
    """The bucket ranges of the data-parallel step (trainer.AEStep.plan) tile each net's flat gradient buffer exactly,
    and every bucket is a contiguous range whose parameters' gradients are final when its all-reduce starts."""
    from zs_amd.model import Decoder, Encoder
    enc = Encoder(c_in=80, c_h1=16, c_h2=32, c_h3=16, ns=0.01, dp=0.5, enc_size=8, seg_len=128, enc_mode='multilabel_binary')
    dec = Decoder(c_in=8, c_out=80, c_h=32, c_a=4, ns=0.01, seg_len=128)
    nd, ne = dec.flat_params()[1].numel(), enc.flat_params()[1].numel()
    d_tail, d_conv, d_emb = dec.flat_range('dense1.weight', 'linear.bias'), dec.flat_range('conv1.weight', 'conv6.bias'), \
        dec.flat_range('input_emb.weight', 'emb5.weight')
    assert d_conv[0] == 0 and d_conv[1] == d_tail[0] and d_tail[1] == d_emb[0] and d_emb[1] == nd
    e_bank, e_rest = enc.flat_range('conv1s.0.weight', 'conv1s.6.bias'), enc.flat_range('conv2.weight', 'linear.bias')
    assert e_bank[0] == 0 and e_bank[1] == e_rest[0] and e_rest[1] == ne
    names = [n for n, _ in dec.named_parameters()]
    lo = names.index('dense1.weight')
    assert names[lo:names.index('input_emb.weight')] == [n for n in names if n.split('.')[0] in
                                                         ('dense1', 'dense2', 'dense3', 'dense4', 'RNN', 'dense5', 'linear')]
    with pytest.raises(ValueError):
        dec.flat_range('linear.bias', 'conv1.weight')


def test_data_parallel_loader_shards_are_disjoint():
    """world 2: rank r serves items [index + r*B, index + (r+1)*B) of each global batch and both advance by world*B -- no item
    is served twice before the wrap; world 1 is the reference's sequence (dataloader.py:43-52)."""
    from zs_amd.dataloader import DataLoader

    class Ids(object):
        def __init__(self, n):
            self.n = n

        def __len__(self):
            return self.n

        def __getitem__(self, i):
            assert 0 <= i < self.n
            return (np.int64(i), np.full((2, 3), i, dtype=np.float32))

    B, n = 4, 100
    loaders = [DataLoader(Ids(n), B, rank=r, world=2) for r in range(2)]
    seen = []
    for step in range(11):                      # 11 global batches of 8 = 88 items: 88 + 16 >= 100 wraps after the 11th
        assert loaders[0].index == loaders[1].index == step * 8
        for dl in loaders:
            seen += next(dl)[0].tolist()
    assert len(seen) == len(set(seen)) == 88 and sorted(seen) == list(range(88))
    next(loaders[0]); next(loaders[1])
    assert loaders[0].index == loaders[1].index == 0          # wrapped together
    single = DataLoader(Ids(n), B)
    ref = []
    for _ in range(5):
        ref += next(single)[0].tolist()
    assert ref == list(range(20))


def test_bench_refuses_a_world_size_that_is_not_gpus():
    """`bench.py --gpus 2` under a 1-rank environment must be an error, not a 1-GPU number labelled n_gpus 2."""
    import subprocess
    env = dict(os.environ, WORLD_SIZE='1', RANK='0', LOCAL_RANK='0')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', '1'], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and 'refusing' in r.stderr and r.stdout.strip() == ''


def test_sanitizer_build_command():
    """ZS_SANITIZE=address: host-side instrumentation only (each -fsanitize= directly after -Xarch_host), separate output."""
    from zs_amd import build as zb
    cmd = zb.command(san='address')
    i = cmd.index('-fsanitize=address')
    assert cmd[i - 1] == '-Xarch_host' and cmd[cmd.index('-o') + 1].endswith('libzs_amd.address.so')
    assert '--offload-arch=gfx950' in cmd
    assert zb.command(san='')[zb.command(san='').index('-o') + 1].endswith('libzs_amd.so')


def test_shard_range():
    from zs_amd.parallel import shard_range
    parts = [shard_range(10, r, 4) for r in range(4)]
    assert parts == [(0, 3), (3, 6), (6, 9), (9, 10)]
    assert sum(b - a for a, b in parts) == 10
