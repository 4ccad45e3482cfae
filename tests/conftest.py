import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


_MIOPEN_ENV = ("MIOPEN_USER_DB_PATH", "MIOPEN_CUSTOM_CACHE_DIR")
_miopen_copy = None


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (runs through the HIP C-ABI)")
    # MIOpen appends every kernel it compiles for a shape the shipped cache lacks (the
    # tests' small and odd shapes) to its cache directory, which monodepth2_amd/__init__.py
    # points at the committed monodepth2_amd/miopen_db: the session (and the processes it
    # starts) works on a scratch copy of it, same contents, so the tree stays as committed
    global _miopen_copy
    if not any(v in os.environ for v in _MIOPEN_ENV):
        import shutil
        import tempfile
        _miopen_copy = tempfile.mkdtemp(prefix="md2_miopen_db_")
        src = os.path.join(REPO, "monodepth2_amd", "miopen_db")
        for f in os.listdir(src):   # contents only: the copies are writable whatever the checkout's modes
            shutil.copyfile(os.path.join(src, f), os.path.join(_miopen_copy, f))
        for v in _MIOPEN_ENV:
            os.environ[v] = _miopen_copy


def pytest_unconfigure(config):
    global _miopen_copy
    if _miopen_copy is not None:
        import shutil
        shutil.rmtree(_miopen_copy, ignore_errors=True)
        for v in _MIOPEN_ENV:
            os.environ.pop(v, None)
        _miopen_copy = None


def pytest_collection_modifyitems(config, items):
    try:
        import torch
        have_gpu = torch.cuda.is_available()
    except Exception:  # pragma: no cover
        have_gpu = False
    if have_gpu:
        return
    skip = pytest.mark.skip(reason="no GPU in this container")
    for item in items:
        if "gpu" in item.keywords:
            item.add_marker(skip)
