"""GPU: registered projections of DBDE16 streams -- dbde16_hip_project_registered (Codec.project_registered16).

tests/test_gpu_registered.py's cases at 16 bits: U16 pixels, one lane per half row, pieces of 120 output columns, U16
max / min planes and U64 per-lane sums of squares.  Every plane, the count and origins_used are compared for equality
with tests/registered_ref.py.
"""
import pytest

from test_gpu_registered import Registered, codec, cus, dv   # noqa: F401  (the cases and the fixtures)

pytestmark = pytest.mark.gpu


class TestRegistered16(Registered):
    BITS = 16
