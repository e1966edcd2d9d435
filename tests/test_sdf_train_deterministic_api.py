"""The deterministic training mode on the sdf_pdf trainer (config 5): the Python switch
(``trainer_sdf.SdfStep(deterministic=...)``, cfg ``train_deterministic``), the header's statement that the
sdf entry points honour the mode, and the workspace sizes (which carry the mode's scratch in both modes
and are computed without a HIP call). No GPU."""
import ctypes
import inspect
import os
import re

from animatable_nerf_amd import _lib, config, trainer_sdf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sdf_step_takes_deterministic():
    sig = inspect.signature(trainer_sdf.SdfStep.__init__)
    assert 'deterministic' in sig.parameters
    assert sig.parameters['deterministic'].default is None


def test_header_says_the_sdf_entry_points_honour_the_mode():
    with open(os.path.join(ROOT, 'include', 'aninerf.h')) as f:
        header = f.read()
    m = re.search(r'/\* anr_train_deterministic:.*?\*/\s*int\s+anr_train_deterministic', header, re.S)
    assert m, 'the comment on anr_train_deterministic is gone'
    text = ' '.join(m.group(0).split())
    assert 'ignores the mode' not in text
    assert 'Not covered: sdf_pdf' not in text
    for name in ('anr_sdf_train_step', 'anr_sdf_network_train_bwd'):
        assert name in text, name


def test_cfg_key_on_the_sdf_subject():
    assert config.subject('anisdf_pdf_s9p').train_deterministic is False
    assert config.subject('anisdf_pdf_s9p', train_deterministic=True).train_deterministic is True


def test_workspace_sizes_are_positive_and_mode_independent(monkeypatch):
    lib = _lib.load()
    o = _lib.RenderOpts()
    o.n_samples, o.chunk = 64, 2048
    sizes = []
    for env in (None, '1', '0'):
        if env is None:
            monkeypatch.delenv('ANR_TRAIN_DETERMINISTIC', raising=False)
        else:
            monkeypatch.setenv('ANR_TRAIN_DETERMINISTIC', env)
        step = int(lib.anr_sdf_train_workspace_bytes(1024, ctypes.byref(o)))
        net = int(lib.anr_sdf_network_train_workspace_bytes(1024 * 64))
        assert step > 0 and net > 0
        sizes.append((step, net))
    assert sizes[0] == sizes[1] == sizes[2]  # the environment can flip the mode per call: one size serves both
