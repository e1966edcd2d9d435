"""The deterministic training mode's switch (include/aninerf.h ``anr_train_deterministic``): declared,
exported, a process-wide 0 / 1 with a query, a rejected bad argument, and the cfg default. No GPU: the
setter makes no HIP call."""
import os
import re

import pytest

from animatable_nerf_amd import _lib, config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_exports_list_it():
    with open(os.path.join(ROOT, 'include', 'aninerf.h')) as f:
        header = f.read()
    assert re.search(r'\bint\s+anr_train_deterministic\s*\(\s*int\s+on\s*\)\s*;', header)
    assert 'anr_train_deterministic' in _lib.EXPORTS
    # the layout limits the mode must respect: no new render option, hooks unchanged
    assert 'deterministic' not in ''.join(n for n, _ in _lib.RenderOpts._fields_)


@pytest.fixture
def lib():
    lib = _lib.load()
    before = lib.anr_train_deterministic(-1)
    yield lib
    lib.anr_train_deterministic(before)


def test_setter_query_round_trip(lib, monkeypatch):
    monkeypatch.delenv('ANR_TRAIN_DETERMINISTIC', raising=False)
    lib.anr_train_deterministic(0)
    assert lib.anr_train_deterministic(-1) == 0  # the default
    assert lib.anr_train_deterministic(1) == 0   # returns the value in force before the call
    assert lib.anr_train_deterministic(-1) == 1
    assert lib.anr_train_deterministic(0) == 1
    assert lib.anr_train_deterministic(-1) == 0


def test_default_is_off_in_a_fresh_process():
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k != 'ANR_TRAIN_DETERMINISTIC'}
    out = subprocess.run([sys.executable, '-c',
                          'from animatable_nerf_amd import _lib; print(_lib.load().anr_train_deterministic(-1))'],
                         cwd=ROOT, env=env, capture_output=True, text=True, check=True)
    assert out.stdout.strip().splitlines()[-1] == '0'


@pytest.mark.parametrize('bad', [2, -2, 7, -100])
def test_bad_argument_is_rejected(lib, bad):
    lib.anr_train_deterministic(1)
    rc = lib.anr_train_deterministic(bad)
    assert rc == -2, rc  # -ANR_E_ARG: negative, never a mode
    assert b'anr_train_deterministic' in lib.anr_last_error()
    assert lib.anr_train_deterministic(-1) == 1  # unchanged


def test_scope_restores_the_previous_mode(lib):
    lib.anr_train_deterministic(0)
    with _lib.deterministic(True):
        assert lib.anr_train_deterministic(-1) == 1
        with _lib.deterministic(False):
            assert lib.anr_train_deterministic(-1) == 0
        with _lib.deterministic(None):
            assert lib.anr_train_deterministic(-1) == 1
        assert lib.anr_train_deterministic(-1) == 1
    assert lib.anr_train_deterministic(-1) == 0


def test_cfg_default():
    assert config.defaults().train_deterministic is False
    assert config.subject('aninerf_313', train_deterministic=True).train_deterministic is True
