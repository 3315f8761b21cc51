"""rainier_amd -- MI355X-native HMC engine behind Rainier's model.sample().

  csrc/            C++ host runtime + hand-written HIP device code -> librainier_hip.so (C ABI: include/rainier_hip.h)
  sampler.py       host-side mirror of the rainier-sampler plugin surface over that C ABI
  frontend.py      small expression DSL that writes RIR (stands in for the JVM front-end in tests/bench)
  models.py        the BASELINE.json configurations as RIR + synthetic data
"""
from .sampler import (Check, Covariance, DefaultConfig, DenseMassMatrixTuner, DensityFunction, DiagonalMassMatrix,  # noqa: F401
                      DiagonalMassMatrixTuner,
                      DualAvgTuner, EHMC, EHMCSampler, Generator, HMC, Histogram, Histogram2d, HMCSampler, IdentityMassMatrixTuner, Loo, LooExpect, LooQuantile, Mcse, Model, NUTSSampler, Ppc, Predictor, RankDiagnostics,
                      RainierHipError, Sampler, SamplerConfig, StaticMassMatrix, StaticStepSize, Summary, Trace, covariance_device,
                      diagnostics, diagnostics_device, format_precis, gen, generate_device, histogram2d_device, histogram_device, loo_compare, loo_device, loo_expect_device, loo_quantile_device, make_config, mcse_device, ppc, ppc_device, predict, predict_device, rank_diagnostics_device, sample_multi,
                      summary_device)
