"""GPU: lag projections of DBDE16 streams -- dbde16_hip_project_lag (Codec.project_lag16).

tests/test_gpu_lag.py's cases at 16 bits: U16 pixels, two pieces across the 200 x 123 frame, one lane per half row, a
U16 maxdiff plane and U64 per-lane product, sqdiff and pairsum.  Every plane and both scalars are compared for equality
with tests/lag_ref.py.
"""
import pytest

from test_gpu_lag import Lag, codec, cus, dv   # noqa: F401  (the cases and the fixtures)

pytestmark = pytest.mark.gpu


class TestLag16(Lag):
    BITS = 16
