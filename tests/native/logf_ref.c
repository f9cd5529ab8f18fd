/* Test helper: the host glibc logf the reference's PGM writer calls
 * (main.cpp:225-235 n_val, `log` of a float under `using namespace std`), so
 * tests can compare ipt_math.h's logf_ and the PGM kernels to it bit-for-bit.
 * Built by tests/pgm_ref.py with gcc -O2 -ffp-contract=off. */
#define _GNU_SOURCE
#include <math.h>
#include <pthread.h>

typedef struct { const float* in; float* out; long lo, hi; } job_t;

static void* run(void* a) {
    job_t* j = (job_t*)a;
    for (long i = j->lo; i < j->hi; ++i) j->out[i] = logf(j->in[i]);
    return 0;
}
void logf_eval(const float* in, float* out, long n, int nthreads) {
    if (nthreads < 1) nthreads = 1;
    if (nthreads > 64) nthreads = 64;
    pthread_t th[64];
    job_t jobs[64];
    for (int t = 0; t < nthreads; ++t) {
        jobs[t].in = in; jobs[t].out = out;
        jobs[t].lo = n * t / nthreads; jobs[t].hi = n * (t + 1) / nthreads;
        pthread_create(&th[t], 0, run, &jobs[t]);
    }
    for (int t = 0; t < nthreads; ++t) pthread_join(th[t], 0);
}
