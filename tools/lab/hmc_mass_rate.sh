# samples/s of the bench's `hmc` object: identity vs diagonal vs dense mass matrix (momenta and energies on the device)
#     bash tools/lab/hmc_mass_rate.sh <output dir>
O=${1:?output dir}
mkdir -p "$O"
for m in identity diag dense identity dense; do
  python bench.py --full --steps 1 --warmup 1 --grad-steps 0 --no-cpu-baseline --hmc-samples 3 --hmc-mass $m > "$O/hmc_$m.json" 2> "$O/hmc_$m.err"
  python -c "import json;r=json.load(open('$O/hmc_$m.json'))['hmc'];print('$m', round(r['samples_per_s'],3), round(r['grad_evals_per_s'],1), r['accept_rate_mean'], r['median_abs_energy_error'])"
done
