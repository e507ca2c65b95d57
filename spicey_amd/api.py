"""The reference's public surface (/root/reference/lib/index.ts:1-12), same names."""
from .ac import formatAcResult, simulateAC  # noqa: F401
from .ac_batch import simulateACBatch  # noqa: F401
from .netlist import parseNetlist  # noqa: F401
from .noise import simulateNoise, simulateNoiseBatch  # noqa: F401
from .simulate import (eecEngineTranToVGraphs, formatTranResult, simulate, simulateTRAN,  # noqa: F401
                       spiceyTranToVGraphs)

__all__ = ["parseNetlist", "simulate", "simulateAC", "simulateACBatch", "simulateNoise", "simulateNoiseBatch", "simulateTRAN", "formatAcResult", "formatTranResult",
           "spiceyTranToVGraphs", "eecEngineTranToVGraphs"]
