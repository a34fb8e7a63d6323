"""Fixture catalogue of the newS test class (classic KM / learned + safeguarded KM of
test_syn_l1l1_newS.py, its _Acols form and the tied / ptied _Acols scripts).

name -> the script, the newS parameter set of `defn` (problems.build_problem), the module globals
the reference class reads (alpha, delta, mu_k_method, mu_k_param, continued) and the forward
arguments (use_learned, use_safeguard, K).  make_golden_news_lskm.py runs the reference class on
each; the tests regenerate the inputs from the definition.
"""
from problems import VARIANT_SPECS, build_problem  # noqa: F401

SCRIPTS = {
    "news": "test_syn_l1l1_newS.py",
    "acols": "test_syn_l1l1_newS_Acols.py",
    "tied": "test_syn_scalar_tied_newS_Acols.py",
    "ptied": "test_syn_scalar_ptied_newS_Acols.py",
}
# the product class of each script and how its fc weights are tied (tests/news_lskm_ref.py)
CLASSES = {"news": "DLADMMNetNewSLSKM", "acols": "DLADMMNetNewSLSKM",
           "tied": "DLADMMNetTiedNewSLSKM", "ptied": "DLADMMNetPTiedNewSLSKM"}
FC = {"news": "per_layer", "acols": "per_layer", "tied": "tied", "ptied": "ptied"}
# every decision of a safeguarded fixture keeps at least this relative distance from its
# threshold in the fp64 run (asserted by the generator, stored in the file)
MIN_MARGIN = 5e-4


def _case(script, defn, layers, K, learned, safeguard, continued=False, alpha=0.01, delta=-99.0,
          mu="None", mu_param=0.0):
    return dict(script=script, defn=defn, layers=layers, K=K, learned=learned,
                safeguard=safeguard, continued=continued, alpha=alpha, delta=delta, mu=mu,
                mu_param=mu_param)


# the newS parameter sets of problems.VARIANT_SPECS (their state_dict keys are the test classes'),
# perturbed; the shapes and seeds of the test_syn_l1l1_scalar.py fixtures
_NS = dict(variant="v7", m=16, n=32, B=24, K=6, seed=1150, perturb=0.3, wscale=0.8)
_NM = dict(variant="v7", m=250, n=500, B=10, K=5, seed=1151, perturb=0.2, wscale=0.9)
# RT / delta 0.1 at the medium shape: with _NM's parameters one fp64 decision sits 1.8e-4 from its
# threshold (below MIN_MARGIN), so this case takes the small fixtures' perturbation instead
_NR = dict(variant="v7", m=250, n=500, B=10, K=5, seed=1151, perturb=0.3, wscale=0.8)
_TS = dict(variant="v7t", m=16, n=32, B=24, K=6, seed=1150, perturb=0.3, wscale=0.8)
_PS = dict(variant="v7p", m=16, n=32, B=24, K=6, seed=1150, perturb=0.3, wscale=0.8, interval=2)

NEWS_LSKM_FIXTURES = {
    "news_lskm_km_small": _case("news", _NS, 6, 120, False, False),       # classic KM only
    "news_lskm_km_med": _case("news", _NM, 5, 60, False, False, alpha=0.05),
    "news_lskm_l2o_small": _case("news", _NS, 6, 6, True, False),         # learned only
    "news_lskm_l2o_med": _case("news", _NM, 5, 5, True, False),
    "news_lskm_sg_ema_small": _case("news", _NS, 6, 6, True, True, delta=0.05, mu="EMA",
                                    mu_param=0.5),
    "news_lskm_sg_rt_small": _case("news", _NS, 6, 6, True, True, delta=0.1, mu="RT"),
    "news_lskm_sg_gs_small": _case("news", _NS, 6, 6, True, True, delta=0.0, mu="GS",
                                   mu_param=0.1),
    "news_lskm_sg_none_small": _case("news", _NS, 6, 6, True, True, delta=0.0),
    "news_lskm_sg_cont_small": _case("news", _NS, 6, 30, True, True, continued=True, delta=0.05,
                                     mu="EMA", mu_param=0.5),
    "news_lskm_sg_ema_med": _case("news", _NM, 5, 5, True, True, delta=0.05, mu="EMA",
                                  mu_param=0.5),
    "news_lskm_sg_rt_med": _case("news", _NR, 5, 5, True, True, delta=0.1, mu="RT"),
    "news_lskm_sg_gs_med": _case("news", _NM, 5, 5, True, True, delta=0.0, mu="GS",
                                 mu_param=0.1),
    "news_lskm_sg_none_med": _case("news", _NM, 5, 5, True, True, delta=0.0),
    "news_lskm_acols_sg_ema": _case("acols", _NS, 6, 6, True, True, delta=0.05, mu="EMA",
                                    mu_param=0.5),
    "news_lskm_tied_km": _case("tied", _TS, 6, 40, False, False),
    "news_lskm_tied_sg_ema": _case("tied", _TS, 6, 6, True, True, delta=0.05, mu="EMA",
                                   mu_param=0.5),
    "news_lskm_tied_sg_rt": _case("tied", _TS, 6, 6, True, True, delta=0.1, mu="RT"),
    "news_lskm_ptied_l2o": _case("ptied", _PS, 6, 6, True, False),
    "news_lskm_ptied_sg_ema": _case("ptied", _PS, 6, 6, True, True, delta=0.05, mu="EMA",
                                    mu_param=0.5),
    "news_lskm_ptied_sg_gs": _case("ptied", _PS, 6, 6, True, True, delta=0.0, mu="GS",
                                   mu_param=0.1),
}
