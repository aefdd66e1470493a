// multi.h -- what api.hip forwards to for a context of a group (multi.hip: gpak_create_multi)
#pragma once
#include <functional>
#include <string>

#include "../../include/gpak_dist.h"
#include "gpak_internal.h"

int gpak_multi_create(gpak_multi **out, int n, const int *devices, int precision, std::string &err,
                      const gpak_dist_engine *const *engines);
void gpak_multi_destroy(gpak_multi *g);
const char *gpak_multi_error(gpak_multi *g);
int gpak_multi_n(gpak_multi *g);
const char *gpak_multi_transport(gpak_multi *g);
int gpak_multi_stats(gpak_multi *g, int r, gpak_dist_stats *out);
int gpak_multi_set_train(gpak_multi *g, const double *X, const double *y, int N, int d);
int gpak_multi_set_params(gpak_multi *g, const double *expans, double bias, double sn2, int dist_mode);
int gpak_multi_set_kernel(gpak_multi *g, int nterms, const int *kinds, const double *pars, double bias, double white,
                          double sn2, int dist_mode);
int gpak_multi_nlz(gpak_multi *g, double *nlz, double *quad, double *sumlp, double *logdet);
int gpak_multi_failed_column(gpak_multi *g);
int gpak_multi_alpha(gpak_multi *g, double *alpha_host);
int gpak_multi_grad(gpak_multi *g, double *grad10);
int gpak_multi_grad_hyb(gpak_multi *g, double *grad, int ng);
int gpak_multi_predict(gpak_multi *g, const double *Xte, long M, int d, double *mean, double *var);
int gpak_multi_timing(gpak_multi *g, gpak_phase_times *out);
// f on the single-GPU context of device 0 (wants_factor: brought up to the ranks' factor first)
int gpak_multi_on_replica0(gpak_multi *g, const std::function<int(gpak_ctx *)> &f, bool wants_factor);
