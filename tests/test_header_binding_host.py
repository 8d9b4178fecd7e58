"""CPU tests of the header-derived binding: ``spkdiff._lib`` reads every signature, the ABI version and the integer macros from
``include/spkdiff.h``.  The reader is checked on synthetic header text (what it must classify, what it must ignore, what it must
refuse by name), then the binding it produced from the real header: every declaration bound, the version, every Python-side
constant against its macro, and the longest signatures written out here argument by argument as the header reads."""
import ctypes
import os
import re
from ctypes import c_char_p, c_float, c_int, c_longlong, c_ulonglong, c_void_p

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spkdiff.h")
P, I, LL, ULL, F = c_void_p, c_int, c_longlong, c_ulonglong, c_float

SYNTHETIC = '''
/* a header in the style of spkdiff.h */
#ifndef FAKE_H
#define FAKE_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
typedef struct ihipStream_t* spk_stream_t; /* == hipStream_t */
#define SPK_VERSION 7 /* a comment
                       * over several lines, with spk_in_macro_comment(int); in it */
int spk_version(void);
const char* spk_error_string(int code);
/* a block comment between declarations: spk_fake(int); and unbalanced ((( parentheses ) */
int spk_many_lines(const float* x_seq, float* v_inout,
                   void* spike_out, int T, long long N,
                   float tau,
                   spk_stream_t stream);
// a line comment: int spk_fake2(double x);
long long spk_pointers(const float* const* list, uint8_t* const* out, void* ws, unsigned* words,
                       const unsigned long long* state, const int *spaced, unsigned long long seed, long long n, float f);
int spk_unnamed(int, float, const void*, spk_stream_t);
#ifdef __cplusplus
}
#endif
#endif
'''


def test_reader_classifies_the_vocabulary_and_ignores_the_rest():
    from spkdiff import _lib
    sigs = _lib.read_signatures(SYNTHETIC)
    assert list(sigs) == ["spk_version", "spk_error_string", "spk_many_lines", "spk_pointers", "spk_unnamed"]   # declaration order
    assert sigs["spk_version"] == (I, [])                                              # a (void) list is empty
    assert sigs["spk_error_string"] == (c_char_p, [I])                                 # const char* return
    assert sigs["spk_many_lines"] == (I, [P, P, P, I, LL, F, P])                       # multi-line; spk_stream_t is a pointer
    # const T* const*, T* const*, void*, unsigned*, const unsigned long long*, `const int *x`: pointers; then the by-value types
    assert sigs["spk_pointers"] == (LL, [P, P, P, P, P, P, ULL, LL, F])
    assert sigs["spk_unnamed"] == (I, [I, F, P, P])
    for res, args in sigs.values():                                                    # the ctypes classes themselves
        assert all(any(a is c for c in (P, I, LL, ULL, F)) for a in args)
    assert sigs["spk_pointers"][1][6] is ctypes.c_ulonglong and sigs["spk_error_string"][0] is ctypes.c_char_p


@pytest.mark.parametrize("decl", [
    "int spk_bad(const float* x, double scale, int n);",                   # by-value double
    "int spk_bad(const float* x, unsigned n);",                            # by-value unsigned
    "int spk_bad(int unsigned);",                                          # (not `int` with a parameter called unsigned)
    "int spk_bad(spk_handle_t h, int n);",                                 # an unknown typedef
    "int spk_bad(int (*callback)(int), int n);",                           # a function pointer
    "int spk_bad(struct spk_opts opts);",                                  # a struct by value
    "int spk_bad;",                                                        # no parameter list
    "int spk_bad();",                                                      # an unspecified list is not (void)
    "double spk_bad(int n);",                                              # a return type outside int / long long / const char*
    "void spk_bad(int n);",
    "float* spk_bad(int n);",
])
def test_reader_refuses_by_name_what_it_cannot_classify(decl):
    from spkdiff import _lib
    text = "int spk_good(int a);\n" + decl + "\nint spk_after(float b);\n"
    with pytest.raises(ValueError, match="spk_bad"):
        _lib.read_signatures(text)
    # never a fallback: the same text without the offending declaration reads cleanly
    assert list(_lib.read_signatures(text.replace(decl, ""))) == ["spk_good", "spk_after"]


def test_reader_refuses_a_second_declaration_of_a_name():
    from spkdiff import _lib
    with pytest.raises(ValueError, match="spk_twice"):
        _lib.read_signatures("int spk_twice(int a);\nint spk_twice(float a);\n")


def test_integer_macros():
    from spkdiff import _lib
    text = ('#ifndef SPK_GUARD_H\n#define SPK_GUARD_H\n#define SPKDIFF_H\n'
            '#define SPK_CHUNK_C4 (-64) /* chunk_out value */\n'
            '#define SPK_MODE_LIF 0    /* BN + LIF -> spikes */\n'
            '#define SPK_VERSION 106 /* 0.1.6 -- a long comment that runs over\n'
            '                         * several lines and names #define SPK_IN_COMMENT 5\n'
            '                         */\n'
            '  #  define SPK_INDENTED 12 // trailing\n'
            '#define SPK_HEX 0x10\n'
            '#define SPK_NEG -3\n'
            '#define SPK_FLOAT 1.5f\n#define SPK_EXPR (SPK_MODE_LIF + 1)\n#define SPK_STR "x"\n#define SPK_CALL(x) 3\n'
            '#define SPK_HALF_OPEN (4\n#define SPK_TWO 1 2\n#define OTHER_NAME 9\n'
            'int spk_version(void);\n#endif\n')
    assert _lib.read_constants(text) == {"SPK_CHUNK_C4": -64, "SPK_MODE_LIF": 0, "SPK_VERSION": 106, "SPK_INDENTED": 12,
                                         "SPK_HEX": 16, "SPK_NEG": -3}
    assert list(_lib.read_signatures(text)) == ["spk_version"]             # macros do not disturb the declarations
    with pytest.raises(TypeError):
        _lib.CONSTANTS["SPK_VERSION"] = 0                                   # read-only


# ---- the real header and library ---------------------------------------------------------------------------------------
def _header_text():
    return re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)


def _header_macro(name):
    """An integer macro of the header, read by a regex of this file's own."""
    m = re.search(r"^#define\s+%s\s+\(?(-?\d+)\)?\s*$" % name, _header_text(), flags=re.M)
    assert m, f"{name} is not an integer macro of include/spkdiff.h"
    return int(m.group(1))


def test_every_declaration_is_bound():
    from spkdiff import _lib
    names = re.findall(r"\b(spk_[a-z0-9_]+)\s*\(", _header_text())           # declaration order
    assert len(names) == len(set(names)) >= 120
    assert _lib.EXPORTS == tuple(names) and len(_lib.EXPORTS) == len(names)
    for n in names:
        fn = getattr(_lib.lib, n)
        assert fn.restype in (I, LL, c_char_p), n
        assert isinstance(fn.argtypes, (list, tuple)) and all(a in (P, I, LL, ULL, F) for a in fn.argtypes), n
    # the argument count of every declaration, counted from the text by its commas
    for m in re.finditer(r"\b(spk_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", _header_text()):
        n_args = 0 if m.group(2).strip() == "void" else m.group(2).count(",") + 1
        assert len(getattr(_lib.lib, m.group(1)).argtypes) == n_args, m.group(1)


def test_version_is_the_headers():
    from spkdiff import _lib
    assert _lib.EXPECTED_VERSION == _header_macro("SPK_VERSION") == _lib.version() == _lib.lib.spk_version()
    assert _lib.CONSTANTS["SPK_VERSION"] == _lib.EXPECTED_VERSION
    assert os.path.samefile(_lib.HEADER_PATH, HEADER)


def test_python_constants_are_the_headers_macros():
    from spkdiff import _lib, ops
    names = {"MODE": ("LIF", "RAW", "MEMOUT", "MEAN"), "IN": ("PTC", "TINV", "SEQ"), "CHUNK": ("C4", "S32"),
             "SPIKE": ("F32", "U8", "BITS"), "LIN_IN": ("F32", "U8", "PTC"), "LIN_OUT": ("F32", "U8", "PTC"),
             "VAE_OUT": ("COLLAPSED", "S32", "PTC")}
    flat = [f"{group}_{n}" for group, members in names.items() for n in members]
    flat += ["STEP_TAIL_MAX_K", "VQ_TRAIN_MAX_D", "VQ_USAGE_MAX_K", "SSIM_MAX_WINDOW"]
    for n in flat:
        assert getattr(ops, n) == _header_macro("SPK_" + n) == _lib.CONSTANTS["SPK_" + n], n
    for group, members in names.items():                                   # an enumeration's members differ
        assert len({getattr(ops, f"{group}_{n}") for n in members}) == len(members), group
    assert (_lib.CONSTANTS["SPK_ERR_ARG"], _lib.CONSTANTS["SPK_ERR_UNSUPPORTED"]) == \
        (_header_macro("SPK_ERR_ARG"), _header_macro("SPK_ERR_UNSUPPORTED")) == (-1, -2)
    # the values every caller of the ABI was built against
    assert (ops.MODE_LIF, ops.MODE_RAW, ops.MODE_MEMOUT, ops.MODE_MEAN) == (0, 1, 2, 3)
    assert (ops.IN_PTC, ops.IN_TINV, ops.IN_SEQ) == (0, 1, 2) and (ops.CHUNK_C4, ops.CHUNK_S32) == (-64, -32)
    assert (ops.SPIKE_F32, ops.SPIKE_U8, ops.SPIKE_BITS) == (0, 1, 2)
    assert (ops.VAE_OUT_COLLAPSED, ops.VAE_OUT_S32, ops.VAE_OUT_PTC) == (0, 1, 2)
    assert (ops.LIN_IN_F32, ops.LIN_IN_U8, ops.LIN_IN_PTC) == (ops.LIN_OUT_F32, ops.LIN_OUT_U8, ops.LIN_OUT_PTC) == (0, 1, 2)
    assert (ops.STEP_TAIL_MAX_K, ops.VQ_TRAIN_MAX_D, ops.VQ_USAGE_MAX_K, ops.SSIM_MAX_WINDOW) == (512, 64, 4096, 31)


def test_error_codes_map_to_exceptions_by_name():
    from spkdiff import _lib
    with pytest.raises(ValueError):
        _lib.check(_header_macro("SPK_ERR_ARG"), "x")
    with pytest.raises(NotImplementedError):
        _lib.check(_header_macro("SPK_ERR_UNSUPPORTED"), "x")
    with pytest.raises(_lib.SpkdiffError):
        _lib.check(1, "x")
    assert _lib.check(0) is None


# The longest signatures, argument by argument as include/spkdiff.h declares them.
PINNED = {
    "spk_den_step_tail_topk": (I, [
        P, I,                        # cnt5, nch5
        P, I,                        # cnt1, nch1
        P, P, P,                     # wq, scale, bias_d
        P, P, P,                     # logits_out_or_null, x_t_inout, unmasked_inout
        I,                           # t
        P, P,                        # temp_b, topk_b
        P, P,                        # u_or_null, q_or_null
        ULL, ULL,                    # philox_seed, philox_offset
        P,                           # philox_state_or_null
        P, P, P, P,                  # conv1_w_packed_or_null, conv1_bias_or_null, bn1_a, bn1_b
        P, P,                        # x1_s32_out_or_null, cnt1_out_or_null
        I, I, I, I, I,               # T, B, H, W, K
        P, P, P]),                   # active_or_null, n_active_or_null, stream
    "spk_conv_train_wgrad": (I, [
        P, P, P, LL, P, P,           # u_cl, v_cl, ws, ws_bytes, gw_out, gb_out_or_null
        I, I, I, I, I, I, I, I, I, I,    # N, Hu, Wu, Cu, Hv, Wv, Cv, k, stride, pad
        LL, LL, LL,                  # g_tap, g_u, g_v
        I, P]),                      # bias_from, stream
    "spk_bn_lif_train_bwd_strided": (I, [
        P, LL, LL,                   # grad_spike_seq, grad_step_stride, grad_row_pitch
        P, P, P, P, P, P, P,         # grad_v_last, y, gamma, beta, save_mean, save_invstd, v_init
        P, P, P, P,                  # grad_y, grad_gamma, grad_beta, grad_v_init
        P, LL,                       # ws, ws_bytes
        I, I, I, I,                  # T, B, C, HW
        F, F, F, F,                  # tau, v_threshold, v_reset, alpha
        I, P]),                      # detach_reset, stream
    "spk_completion_state": (I, [
        P, P, P, P, P,               # codes_bhw, keep_mask, x_t_out, unmasked_out, n_known_out_or_null
        I, I, I, I, I, I, I, I,      # B, h, w, Hm, Wm, stride, radius, K
        LL, P]),                     # mask_id, stream
    "spk_error_string": (c_char_p, [I]),
}


@pytest.mark.parametrize("name", sorted(PINNED))
def test_longest_signatures_in_full(name):
    from spkdiff import _lib
    fn = getattr(_lib.lib, name)
    res, args = PINNED[name]
    assert fn.restype is res
    assert len(fn.argtypes) == len(args)
    assert [i for i, (a, b) in enumerate(zip(fn.argtypes, args)) if a is not b] == []


def test_pinned_signatures_have_the_shape_the_header_shows():
    assert len(PINNED["spk_den_step_tail_topk"][1]) == 32 and PINNED["spk_den_step_tail_topk"][1].count(ULL) == 2
    assert PINNED["spk_conv_train_wgrad"][1][6:19] == [I] * 10 + [LL] * 3
    assert PINNED["spk_bn_lif_train_bwd_strided"][1][1:3] == [LL, LL] and PINNED["spk_bn_lif_train_bwd_strided"][1].count(F) == 4
    assert PINNED["spk_completion_state"][1][13] is LL
