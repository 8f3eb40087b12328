/* Dev aid (not product): accuracy of the binary64 exp form of the fog term (device_math.h exp_spec; its CPU statement is
 * tests/fog_checker.c skf_exp_spec, compared with the device bit for bit by tests/test_fog_gpu.py) over EVERY binary32 argument whose
 * exp is a finite non-zero binary32 — the arguments blinn_phong.h:27 forms are binary32 and the result is narrowed to binary32 —,
 * against expl (x87 extended, 11 bits beyond binary64).  Reports the largest error in binary64 ulps and how many narrowed results
 * differ from the correctly rounded binary32 exp.
 * Build and run:  gcc -O2 -fopenmp -ffp-contract=off -mfma -shared -fPIC -o /tmp/libfogcheck.so tests/fog_checker.c -Loracle -l:liboracle.so -lm &&
 *                 gcc -O2 -fopenmp -o /tmp/exp_exhaustive tools/exp_exhaustive.c /tmp/libfogcheck.so -Loracle -l:liboracle.so -lm &&
 *                 LD_LIBRARY_PATH=oracle:/tmp /tmp/exp_exhaustive */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
double skf_exp_spec(double x);
static inline float asf(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
int main(void)
{
	double worst = 0, worst_x = 0;
	uint64_t n = 0, narrowed_off = 0;
#pragma omp parallel for schedule(dynamic, 1 << 16) reduction(+ : n, narrowed_off)
	for(int64_t u = 0; u < (int64_t) 1 << 32; u++)
	{
		const float x = asf((uint32_t) u);
		if(!(x >= -104.0f && x <= 88.8f)) continue;
		const double got = skf_exp_spec((double) x);
		const long double want = expl((long double) x);
		const float fw = (float) want;
		if(fw == 0.0f || isinf(fw)) continue;
		n++;
		const double w = (double) want;
		const double ulp = nextafter(w, INFINITY) - w;
		const double err = (double) fabsl((long double) got - want) / ulp;
		narrowed_off += ((float) got != fw);
#pragma omp critical
		if(err > worst) { worst = err; worst_x = x; }
	}
	printf("binary32 arguments: %llu; max error %.4f ulp of binary64 (at x = %a); narrowed results != correctly rounded binary32: %llu\n",
		   (unsigned long long) n, worst, worst_x, (unsigned long long) narrowed_off);
	return 0;
}
