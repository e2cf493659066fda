import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
# the reference's test data the suite reads (example model sets, model files, PMML fixtures):
# data files only, packed into one archive; reference_resources.MANIFEST lists its contents
REF_ARCHIVE = os.path.join(ROOT, "tests", "golden", "reference_resources.tar.gz")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs an MI355X (HIP kernels)")
    config.addinivalue_line("markers", "slow: long-running")


def pytest_collection_modifyitems(config, items):
    import torch
    if torch.cuda.is_available():
        return
    skip = pytest.mark.skip(reason="no GPU")
    for it in items:
        if "gpu" in it.keywords:
            it.add_marker(skip)


@pytest.fixture(autouse=True)
def _restore_environ():
    """Several CPU tests set SHIFU_FORCE_CPU (and the like) in os.environ directly: put the
    environment back after every test, so a GPU test that follows in the same process runs on
    the GPU."""
    saved = dict(os.environ)
    yield
    for k in set(os.environ) - set(saved):
        del os.environ[k]
    os.environ.update(saved)


@pytest.fixture(scope="session")
def ref_resources(tmp_path_factory):
    import tarfile
    dst = tmp_path_factory.mktemp("reference_resources")
    with tarfile.open(REF_ARCHIVE) as tar:
        for m in tar.getmembers():
            assert (m.isfile() or m.isdir()) and not os.path.isabs(m.name) and ".." not in m.name.split("/"), m.name
        tar.extractall(dst)
    return str(dst)
