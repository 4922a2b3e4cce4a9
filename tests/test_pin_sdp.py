"""tools/pin_sdp.py runs the reference's OWN ``SDP.identifyFeasibleStandardParameters`` (identification/sdp.py:450-604), unmodified, fed
once by its own ``la.qr(YBase)`` and once by the TSQR factor of the path (``estimation.sdp_inputs``), xStd compared at 1e-6.  That run needs
a checkout of the reference (``--reference DIR``), which is not part of this repository; the suite only holds the tool to its contract
when the checkout is missing."""
import os
import sys

from common import ROOT


def test_tool_reports_what_is_missing(tmp_path):
    """Without cvxpy / a device the tool says so and exits with 3 ("not pinned"), never with a traceback or a false 0."""
    import subprocess

    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "pin_sdp.py"), "--reference", str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 3 and "missing" in r.stderr and "reference checkout" in r.stderr

