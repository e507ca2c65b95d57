"""spicey_amd — MI355X-native drop-in for tscircuit/spicey's simulation paths.

`spicey_amd.api` carries the public names of /root/reference/lib/index.ts:1-12 (parseNetlist, simulate, simulateAC,
simulateTRAN, formatAcResult, formatTranResult, spiceyTranToVGraphs, eecEngineTranToVGraphs).  The solvers (transient
and AC) run in libspicey_hip.so (include/spicey_hip.h); nothing here computes on the CPU.  Importing this package does
not load the library: spicey_amd.lib does on first use, and fails loudly when it is missing.

Beyond the reference's surface: measureTRAN / measureTRANBatch (spicey_amd.measure) reduce a transient to a few numbers
per circuit on the device instead of returning every sample — extremes, averages and crossings (stats, cross),
harmonics with THD (fourier) and edge timing (when, delay, rise_time, fall_time, settle); simulateACBatch (spicey_amd.ac_batch) runs many circuits' AC
sweeps as the instances of one launch, and measureAC / measureACBatch (spicey_amd.ac_measure) reduce such sweeps on the
device to corner frequencies, peaks and point read-outs; simulateNoise / simulateNoiseBatch (spicey_amd.noise) run one sweep
with a current injected at the output and reduce it on the device to output impedance, gain, thermal noise and the resistors'
shares of it; simulateSens / simulateSensBatch (spicey_amd.sens) run that sweep and the plain one and reduce the two on the
device to every element's first-order sensitivity of magnitude and phase and to worst-case and root-sum-square tolerance bounds;
simulateMonteCarlo (spicey_amd.mc) draws the samples of a tolerance analysis on the device, sweeps them as the instances of one
launch and reduces them across the instances to quantile bands, moments and the yield against a spec mask;
measureMonteCarlo (spicey_amd.tran_mc) does the same for transient runs: the samples are the instances of one transient, and the
scalars of measureTRAN's measures are reduced across them to quantiles, moments, yields against limits and the worst samples;
measureSens / measureWorstCase (spicey_amd.tran_sens) perturb one toleranced element at a time, as the instances of one transient,
reduce the scalars across them to every element's first-order sensitivity and curvature and to worst-case and root-sum-square
bounds, and run the tolerance corners the signs point to as the instances of a second one;
steadyState / steadyStateBatch (spicey_amd.pss) find the periodic steady state of a driven circuit by shooting Newton — the
nominal and the state-perturbed copies are the instances of one transient over one period, the dense update runs on the device —
and write it into the circuit, so that the next analysis starts there;
optimizeTRAN / optimizeTRANBatch (spicey_amd.fit) size elements so that transient measurements meet goals: a damped
least-squares loop over element gains whose Jacobian is the one-at-a-time design of measureSens, updated on the device.
"""
from .ac_batch import simulateACBatch  # noqa: F401
from .ac_measure import measureAC, measureACBatch  # noqa: F401
from .noise import simulateNoise, simulateNoiseBatch  # noqa: F401
from .sens import simulateSens, simulateSensBatch  # noqa: F401
from .mc import mc_values, simulateMonteCarlo  # noqa: F401
from .tran_mc import measureMonteCarlo  # noqa: F401
from .tran_sens import design_circuit, measureSens, measureWorstCase  # noqa: F401
from .pss import steadyState, steadyStateBatch  # noqa: F401
from .fit import at_least, at_most, between, optimizeTRAN, optimizeTRANBatch, target  # noqa: F401
from .measure import deriv, efficiency, find, measureTRAN, measureTRANBatch, power, sample, trace  # noqa: F401
