# Top-level build: the HIP E-step library (gfx950), the oracle (C restatement,
# test infrastructure), and the test-only MATLAB API double + MEX gateway.
PKG      := clustering-hidden-markov-models-with-variational-bayesian-hierarchical-em_amd
HIPCC    ?= /opt/rocm/bin/hipcc
ARCH     ?= gfx950
HIPFLAGS ?= --offload-arch=$(ARCH) -O3 -fPIC -std=c++17 -Wall -Wno-unused-function
LIBDIR   := $(PKG)/lib
SRCS     := $(PKG)/csrc/vbhem_kernels.hip $(PKG)/csrc/vbhem_fb_split.hip $(PKG)/csrc/vbhem_fb_bwd.hip $(PKG)/csrc/vbhem_fb_bwd4.hip $(PKG)/csrc/vbhem_fb_bwd12.hip $(PKG)/csrc/vbhem_fb_list4.hip $(PKG)/csrc/vbhem_fb_list12.hip $(PKG)/csrc/vbhem_emission.hip $(PKG)/csrc/vbhem_stats.hip $(PKG)/csrc/vbhem_capi.hip $(PKG)/csrc/vbhem_em.hip $(PKG)/csrc/vbhem_em_dev.hip $(PKG)/csrc/vbhem_rccl.hip $(PKG)/csrc/vbhem_h3m.hip $(PKG)/csrc/vbhmm_fb.hip $(PKG)/csrc/vbhmm_score.hip $(PKG)/csrc/vbhmm_ppk.hip $(PKG)/csrc/vbhmm_ccfd.hip $(PKG)/csrc/vbhmm_dic.hip $(PKG)/csrc/vbhmm_em.hip
HDRS     := include/vbhem_estep.h include/vbhem_dist.h include/vbhmm_fb.h $(PKG)/csrc/vbhem_internal.h $(PKG)/csrc/vbhem_switches.h $(PKG)/csrc/vbhem_math.h $(PKG)/csrc/vbhem_log_table.h include/vbhem_em.h $(PKG)/csrc/vbhem_em_dev.h $(PKG)/csrc/vbhem_exact.h $(PKG)/csrc/vbhem_mfma4.h include/vbhmm_score.h $(PKG)/csrc/vbhmm_score_pair.h include/vbhmm_ppk.h $(PKG)/csrc/vbhmm_ppk_pair.h include/vbhmm_ccfd.h $(PKG)/csrc/vbhmm_ccfd_row.h include/vbhmm_dic.h $(PKG)/csrc/vbhmm_dic_pair.h include/vbhmm_em.h $(PKG)/csrc/vbhmm_em_run.h
OBJS     := $(patsubst $(PKG)/csrc/%.hip,$(LIBDIR)/%.o,$(SRCS))

all: lib oracle mex mathcheck scorecheck ppkcheck ccfdcheck diccheck vbhmmemcheck

lib: $(LIBDIR)/libvbhem_estep.so

$(LIBDIR)/%.o: $(PKG)/csrc/%.hip $(HDRS)
	@mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -Iinclude -I$(PKG)/csrc -c -o $@ $<

$(LIBDIR)/libvbhem_estep.so: $(OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(OBJS)

oracle:
	$(MAKE) -C oracle liboracle.so

# test-only: a MATLAB mx/mex API double and the MEX gateway built against it
mex: tests/mxshim/libmxshim.so $(LIBDIR)/vbhem_hmm_bwd_fwd_mex.so $(LIBDIR)/hem_hmm_bwd_fwd_mex.so $(LIBDIR)/vbhmm_fb_mex.so $(LIBDIR)/vbhem_estep_fused_mex.so

tests/mxshim/libmxshim.so: tests/mxshim/mxshim.c tests/mxshim/mex.h
	gcc -O2 -fPIC -shared -Itests/mxshim -o $@ $<

$(LIBDIR)/%_mex.so: integration/%_mex.c integration/h3m_mex_common.h include/vbhem_estep.h include/vbhmm_fb.h $(LIBDIR)/libvbhem_estep.so tests/mxshim/mex.h
	gcc -O2 -fPIC -shared -Iinclude -Itests/mxshim -Iintegration -o $@ $< -L$(LIBDIR) -lvbhem_estep -lm -Wl,-rpath,'$$ORIGIN'

# test-only: the restricted-domain exp/log/rcp of vbhem_math.h, host and device
mathcheck: tests/mathcheck/libmathcheck.so

tests/mathcheck/libmathcheck.so: tests/mathcheck/mathcheck.hip $(PKG)/csrc/vbhem_math.h $(PKG)/csrc/vbhem_log_table.h $(PKG)/csrc/vbhem_mfma4.h
	$(HIPCC) $(HIPFLAGS) -I$(PKG)/csrc -shared -o $@ $<

# test-only: the sequence-scoring pair routines of vbhmm_score_pair.h on the host, and
# the library's scoring kernels behind the same call
scorecheck: tests/scorecheck/libscorecheck.so

tests/scorecheck/libscorecheck.so: tests/scorecheck/scorecheck.hip $(PKG)/csrc/vbhmm_score_pair.h include/vbhmm_score.h include/vbhmm_fb.h include/vbhem_estep.h $(LIBDIR)/libvbhem_estep.so
	$(HIPCC) $(HIPFLAGS) -Iinclude -I$(PKG)/csrc -shared -o $@ $< -L$(LIBDIR) -lvbhem_estep -Wl,-rpath,'$$ORIGIN/../../$(LIBDIR)'

# test-only: the probability product kernel routines of vbhmm_ppk_pair.h on the host, and
# the library's Gram-matrix kernels behind the same call
ppkcheck: tests/ppkcheck/libppkcheck.so

tests/ppkcheck/libppkcheck.so: tests/ppkcheck/ppkcheck.hip $(PKG)/csrc/vbhmm_ppk_pair.h $(PKG)/csrc/vbhmm_score_pair.h include/vbhmm_ppk.h include/vbhmm_score.h include/vbhmm_fb.h include/vbhem_estep.h $(LIBDIR)/libvbhem_estep.so
	$(HIPCC) $(HIPFLAGS) -Iinclude -I$(PKG)/csrc -shared -o $@ $< -L$(LIBDIR) -lvbhem_estep -Wl,-rpath,'$$ORIGIN/../../$(LIBDIR)'

# test-only: the density-peak row routines of vbhmm_ccfd_row.h and the CCFD distance over
# pair_loglik on the host, and the library's CCFD kernels behind the same calls
ccfdcheck: tests/ccfdcheck/libccfdcheck.so

tests/ccfdcheck/libccfdcheck.so: tests/ccfdcheck/ccfdcheck.hip $(PKG)/csrc/vbhmm_ccfd_row.h $(PKG)/csrc/vbhmm_score_pair.h include/vbhmm_ccfd.h include/vbhmm_score.h include/vbhmm_fb.h include/vbhem_estep.h $(LIBDIR)/libvbhem_estep.so
	$(HIPCC) $(HIPFLAGS) -Iinclude -I$(PKG)/csrc -shared -o $@ $< -L$(LIBDIR) -lvbhem_estep -Wl,-rpath,'$$ORIGIN/../../$(LIBDIR)'

# test-only: the pair routine of vbhmm_dic_pair.h on the host, and the library's DIC
# likelihood kernels behind the same call
diccheck: tests/diccheck/libdiccheck.so

tests/diccheck/libdiccheck.so: tests/diccheck/diccheck.hip $(PKG)/csrc/vbhmm_dic_pair.h $(PKG)/csrc/vbhem_math.h include/vbhmm_dic.h include/vbhem_estep.h $(LIBDIR)/libvbhem_estep.so
	$(HIPCC) $(HIPFLAGS) -Iinclude -I$(PKG)/csrc -shared -o $@ $< -L$(LIBDIR) -lvbhem_estep -Wl,-rpath,'$$ORIGIN/../../$(LIBDIR)'

# test-only: the serial walker over the run routines of vbhmm_em_run.h on the host, and the
# library's batched EM kernels behind the same call
vbhmmemcheck: tests/vbhmmemcheck/libvbhmmemcheck.so

tests/vbhmmemcheck/libvbhmmemcheck.so: tests/vbhmmemcheck/vbhmmemcheck.hip $(PKG)/csrc/vbhmm_em_run.h include/vbhmm_em.h include/vbhmm_fb.h include/vbhem_estep.h $(LIBDIR)/libvbhem_estep.so
	$(HIPCC) $(HIPFLAGS) -Iinclude -I$(PKG)/csrc -shared -o $@ $< -L$(LIBDIR) -lvbhem_estep -Wl,-rpath,'$$ORIGIN/../../$(LIBDIR)'

# test-only, CPU: the serial walker in a stand-alone program under the address and
# undefined-behaviour sanitizers (not part of `all`, not run by pytest)
vbhmmem_sanitize: tests/vbhmmemcheck/walker_main.cpp $(PKG)/csrc/vbhmm_em_run.h
	$(CXX) -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Wall -I$(PKG)/csrc -o tests/vbhmmemcheck/walker_sanitize $<
	tests/vbhmmemcheck/walker_sanitize

clean:
	rm -f $(LIBDIR)/*.o $(LIBDIR)/*.so tests/mxshim/libmxshim.so tests/mathcheck/libmathcheck.so tests/scorecheck/libscorecheck.so tests/ppkcheck/libppkcheck.so tests/ccfdcheck/libccfdcheck.so tests/diccheck/libdiccheck.so tests/vbhmmemcheck/libvbhmmemcheck.so tests/vbhmmemcheck/walker_sanitize
	$(MAKE) -C oracle clean

.PHONY: all lib oracle mex mathcheck scorecheck ppkcheck ccfdcheck diccheck vbhmmemcheck vbhmmem_sanitize clean
