"""Source time functions for WaveEquation.step (include/smg.h: smg_wave_step): values of a wavelet at the step times, to be placed in the signal
(n_steps + 1) x n_src x k.  These functions are data: the one kernel k_wave_sources adds whatever signal it is given."""
import numpy as np


def ricker(f0, t, t0):
    """the Ricker wavelet (1 - 2 a) exp(-a), a = (pi f0 (t - t0))^2, of peak frequency f0 centred at t0, at the times t"""
    a = (np.pi * f0 * (np.asarray(t, dtype=np.float64) - t0)) ** 2
    return (1.0 - 2.0 * a) * np.exp(-a)
