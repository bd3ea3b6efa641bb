"""Option gen_conv_precision / iodine_op_gen_conv_f16x3 (kernels_gensplit.hip): what can be checked without a GPU - the header documents
what the library gained, the built library exports the entry point, the build lists the source, the engine takes the flag."""
import ctypes
import os
import re

from iodine_amd import _lib, build, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, 'include', 'iodine_hip.h')).read()


def test_header_declares_the_entry_point_and_documents_option_and_category():
    assert re.search(r'\bint\s+iodine_op_gen_conv_f16x3\s*\(', HEADER)
    assert '"gen_conv_precision"' in HEADER and '"gen_conv_f16x3"' in HEADER
    assert 'any stride s in {1, 2}' not in HEADER                      # the stale sentence of iodine_op_gen_conv


def test_built_library_exports_the_entry_point():
    assert 'iodine_op_gen_conv_f16x3' in _lib.EXPORTS
    lib = ctypes.CDLL(build.LIB)
    assert hasattr(lib, 'iodine_op_gen_conv_f16x3')


def test_build_lists_the_new_source():
    assert 'kernels_gensplit.hip' in build.SOURCES
    assert os.path.exists(os.path.join(build.CSRC, 'kernels_gensplit.hip'))


def test_engine_parser_accepts_the_flag():
    ap = engine.make_parser()
    assert ap.parse_args(['--gen-conv-precision', '1']).gen_conv_precision == 1
    assert ap.parse_args([]).gen_conv_precision == 0
