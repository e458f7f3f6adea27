"""What the compute kernels share through csrc/lds_dma.h, and the strip kernels among them through csrc/strip_conv.h, stays in
those headers: the Makefile rebuilds their users (both element types) when one changes, and none of them grows a private copy of
its helpers again (source text only, no GPU)."""
import os
import re

from conftest import ROOT

CSRC = os.path.join(ROOT, 'rmem_ocu_amd', 'csrc')
USERS = ('gemm_conv', 'bottleneck', 'bneck_block', 'stem', 'conv3x3_direct', 'idbank', 'rowchain')
HELPERS = ('make_rsrc', 'buf_load_lds16', 'swz')
STRIP_USERS = ('conv3x3_direct', 'bneck_block', 'stem')
STRIP_HELPERS = ('ring3x3_mfma', 'ring_slot_off', 'strip_runs')


def _definitions(text, name):
    """how many functions called `name` the text defines at namespace scope (a line that starts a declaration and opens a body)"""
    return len(re.findall(r'^(?!//)\S.*\b\w+[ *&]+%s\s*\([^;]*\{' % name, text, re.M))


def _prerequisites(makefile, target):
    """every prerequisite that the explicit rules (no recipe, no pattern) of the Makefile give `target`"""
    found = set()
    for line in makefile.split('\n'):
        if line.startswith(('\t', '#')) or ':' not in line or '=' in line or '%' in line:
            continue
        targets, prereqs = line.split(':', 1)
        if target in targets.split():
            found.update(prereqs.split())
    return found


def test_makefile_rebuilds_the_users_of_lds_dma_h():
    makefile = open(os.path.join(CSRC, 'Makefile')).read()
    for stem in USERS:
        for obj in (stem + '.o', stem + '_f16.o'):
            assert 'lds_dma.h' in _prerequisites(makefile, obj), obj
        assert stem + '.hip' in makefile.split('KSRCS')[1].split('\n')[0]


def test_users_include_the_header_and_define_no_copy():
    for stem in USERS:
        text = open(os.path.join(CSRC, stem + '.hip')).read()
        assert text.count('#include "lds_dma.h"') == 1, stem
        for name in HELPERS:
            assert _definitions(text, name) == 0, (stem, name)


def test_header_defines_each_helper_once():
    text = open(os.path.join(CSRC, 'lds_dma.h')).read()
    assert '__global__' not in text
    assert _definitions(text, 'make_rsrc') == 2               # the device pass's, and its empty twin for the host pass
    assert _definitions(text, 'buf_load_lds16') == 2
    assert _definitions(text, 'swz') == 1                     # plain arithmetic: one definition serves both passes
    assert len(re.findall(r'^constexpr int OOB\b', text, re.M)) == 1


def test_makefile_rebuilds_the_users_of_strip_conv_h():
    makefile = open(os.path.join(CSRC, 'Makefile')).read()
    for stem in STRIP_USERS:
        for obj in (stem + '.o', stem + '_f16.o'):
            assert 'strip_conv.h' in _prerequisites(makefile, obj), obj


def test_strip_kernels_include_strip_conv_h_and_define_no_copy():
    for stem in STRIP_USERS:
        text = open(os.path.join(CSRC, stem + '.hip')).read()
        assert text.count('#include "strip_conv.h"') == 1, stem
        for name in STRIP_HELPERS:
            assert _definitions(text, name) == 0, (stem, name)


def test_strip_conv_h_defines_each_helper_once():
    text = open(os.path.join(CSRC, 'strip_conv.h')).read()
    assert '__global__' not in text
    for name in STRIP_HELPERS:
        assert _definitions(text, name) == 1, name
