import os
import sys

import pytest

# a kernel fault should end the test run, not spend minutes writing a GPU core dump first (must be set before the runtime starts)
os.environ.setdefault("HSA_DISABLE_COREDUMP_ON_EXCEPTION", "1")
# torch's CPU BLAS is MKL.  Outside its conditional-numerical-reproducibility mode MKL picks a summation order by CPU make, and
# on an AMD EPYC host that order moved a first moment of test_g3_three_adam_steps 3 % past its bound against the golden
# vectors; in that mode (MKL_CBWR=AUTO: the CPU's own branch) the suite passes on the Intel and AMD hosts it was run on.  MKL
# reads the setting at its first call, so it is made before any test runs a torch op
os.environ.setdefault("MKL_CBWR", "AUTO")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture(scope="session")
def cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _attribute_async_gpu_errors(request):
    """Launches are asynchronous: a fault raised by one test's kernels would otherwise surface at the first host
    synchronisation of a LATER test.  Synchronising after every GPU test pins it to the test that caused it."""
    yield
    if request.node.get_closest_marker("gpu") is not None:
        import torch
        if torch.cuda.is_available():
            torch.cuda.synchronize()
