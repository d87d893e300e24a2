// hydra_main.cpp -- `hydra_mi355x`: hydra's command line on top of the C ABI.
//
// Drop-in for `hydra --mpibayes bayesMPI --bfile X --pheno P ...`
// (src/main.cpp:17-195 -> BayesRRm::runMpiGibbs, src/BayesRRm.cpp:933): same
// flags (src/options.cpp:7-297; defaults src/options.hpp:101-127), same input
// files (.bed/.bim/.fam, .phen with NA, --groupIndexFile/--groupMixtureFile),
// same output files and byte layouts (src/BayesRRm.cpp:1071-1083,1299-1309,
// 2736-2794): <dir>/<name>.csv .bet .cpn .acu .mus.<rank>, and on --save
// .eps.<rank> .mrk.<rank> .rng.<rank> .xbet .xcpn (:2802-2838); --restart
// [--ignore-xfiles] resumes from those dumps into <name>_rs.* (:842-928,
// :1197-1220).
//
// `--mpibayes bayesWMPI --failure F --quad_points Q` runs BayesW (src/BayesW.cpp:905), sharded the same way.
//
// `--predict-bfile T [--predict-out F] [--predict-dry-run]` appended to a bayesMPI command line samples nothing: it scores the target
// cohort T with the chain's .bet records at or after --burn-in (run_predict); the dry run stops after every
// check and the marker-match report, before the device.
//
// `--ld-window W [--ld-window-kb KB] [--ld-window-r2 T] [--ld-out F] [--ld-bin]` appended to a bayesMPI command line samples nothing
// either: it computes r between every marker and the next W markers of its chromosome (within KB kilobases when given) on the chain's
// own rows and standardisation, with hgibbs_ld (run_ld), and writes the pairs with r^2 >= T as PLINK's --r
// table to <dir>/<name>.ld (or F), and with --ld-bin the whole band as f32 to <out>.bin.
//
// `--assoc [--assoc-no-loco] [--assoc-out F]` appended to a bayesMPI command line samples nothing either: it tests every marker for
// association on the chain's rows, against the scaled phenotype minus the chain's genetic value from the other chromosomes (LOCO
// offsets from the .bet records at or after --burn-in; none with --assoc-no-loco), with the covariates projected out, through
// hgibbs_score and hgibbs_marker_dots (run_assoc), and writes <dir>/<name>.assoc (or F).  With --assoc-logistic
// the phenotype is case/control and the table is the logistic score test: a null model per chromosome on [1 | covariates | G - G_c]
// (hgibbs_logit_null) and the sums of its vectors over the rows of each genotype through hgibbs_marker_class_sums
// (run_assoc_logistic), written to <dir>/<name>.assoc.logistic (or F).  `--assoc-spa [--assoc-spa-sd T]` with it replaces P by a
// saddlepoint approximation for the markers whose score is more than T (default 2) SD from 0 and adds the columns P_NORM and SPA
// (hgibbs_spa_roots, hgibbs_spa_pvalue).  `--assoc-firth [--assoc-firth-p T]` with it (and without --assoc-spa) refits
// the markers whose score-test P is at most T (default 0.05) with Firth's penalised likelihood, writes BETA, SE, CHISQ and P from that fit
// and adds the columns P_NORM, BETA_SCORE, SE_SCORE and FIRTH (hgibbs_firth_fit, hgibbs_firth_stats).
// `--assoc-sets FILE [--assoc-set-beta A B] [--assoc-set-maf X] [--assoc-set-out F]` with --assoc-logistic also tests the marker sets of
// FILE (SETNAME SNPID, --pve-sets' format): burden and SKAT from the plain scores and their joint covariance under the null model
// (hgibbs_set_gram, hgibbs_set_tests), written to <dir>/<name>.assoc.sets (or F).
//
// `--king [--king-cutoff T] [--king-out F]` appended to a bayesMPI command line samples nothing either: it computes the KING-robust
// kinship of every pair of the chain's rows with hgibbs_king_pairs (run_king) and writes the pairs with
// KINSHIP >= T (default 0.0442) to <dir>/<name>.kin0 (or F).
//
// `--pca K [--pca-iters P] [--pca-tol T] [--pca-out F] [--pca-loadings]` appended to a bayesMPI command line samples nothing either: it
// computes the K leading principal components of the chain's rows with hgibbs_pca (run_pca), seeded by --seed,
// and writes <dir>/<name>.eigenvec (or F), .eigenval, a .cov file that --covariates reads as it stands and, with --pca-loadings, .var.
//
// `--pve [--pve-window-kb KB | --pve-window-snps W | --pve-sets F | --pve-groups] [--pve-threshold T] [--pve-out F] [--pve-bin]` appended
// to a bayesMPI command line samples nothing either: for every marker set (one per chromosome when none is defined) and every .bet record
// at or after --burn-in it takes the variance over the chain's rows of the set's genetic value with hgibbs_region_var (run_pve,
// DESIGN.md section 18) and writes posterior mean and sd of the variance explained, its share of the genetic variance and the window
// posterior probability of association to <dir>/<name>.pve (or F), and with --pve-bin the variances themselves to <out>.bin.
//
// `--grm [--grm-out PREFIX] [--grm-sparse T]` appended to a bayesMPI command line samples nothing either: it computes the genomic
// relationship matrix of the chain's rows, A = X X' / NSNP on the chain's own standardisation, with hgibbs_grm (run_grm, DESIGN.md
// section 19) and writes GCTA's PREFIX.grm.id, .grm.bin and .grm.N.bin (PREFIX defaults to <dir>/<name>), and with --grm-sparse the
// diagonal and the pairs with A >= T to PREFIX.grm.sp.
//
// `--ld-score [--ld-score-kb KB | --ld-score-snps W] [--ld-score-sets F | --ld-score-groups] [--ld-score-raw] [--ld-score-out PREFIX]`
// appended to a bayesMPI command line samples nothing either: it computes the LD score of every marker, the sum of the adjusted r^2 (raw
// with --ld-score-raw) over the markers of its chromosome within KB kilobases (default 1000) or W markers on either side, on the chain's
// own rows and standardisation, with hgibbs_ld_scores (run_ldscore), partitioned by the sets of F or the groups of
// --groupIndexFile behind a `base` column, and writes LDSC's PREFIX.l2.ldscore, .l2.M and .l2.M_5_50 as plain text (PREFIX defaults to
// <dir>/<name>).  Not covered: cM windows, gzip, the regression itself (ldsc reads these files).
//
// `--clump FILE [--clump-p1 P1] [--clump-p2 P2] [--clump-r2 R2] [--clump-kb KB | --clump-snps W] [--clump-snp-field NAME] [--clump-field NAME]
// [--clump-out F]` appended to a bayesMPI command line samples nothing either: it turns the table FILE of per-marker P values (the .assoc
// of --assoc as it stands) into independent signals, PLINK's clump walk on the chain's own rows and standardisation: hgibbs_ld_mask reduces
// the band to one bit per pair (r^2 >= R2 within KB kilobases, default 250, or W markers), hgibbs_ld_greedy walks the markers with P <= P2
// by ascending P, those with P <= P1 lead (run_ldselect); <dir>/<name>.clumped (or F) has PLINK's columns.
//
// `--ld-prune T [--ld-prune-kb KB | --ld-prune-snps W] [--ld-prune-out PREFIX]` appended to a bayesMPI command line samples nothing either:
// the same walk over every marker with a finite sd by descending minor allele frequency keeps a maximal set without a pair of r^2 > T
// inside the window (default 50 markers) and writes PREFIX.prune.in and PREFIX.prune.out (PREFIX defaults to <dir>/<name>).
//
// `--he [--he-out F] [--he-rows]` appended to a bayesMPI command line samples nothing either: it estimates the SNP heritability of the
// chain's scaled phenotype (with --covariates, [1 | covariates] projected out as --assoc does and scaled again) by Haseman-Elston
// regression on the off-diagonal entries of the relationship matrix of --grm, which never leaves the device: hgibbs_grm_rowsums reduces it
// to a few sums per row, hgibbs_he_fit fits HE-CP and HE-SD with OLS and delete-one-individual jackknife standard errors (run_he,
// DESIGN.md section 22).  <dir>/<name>.HEreg (or F) has the layout of GCTA's --HEreg; with --he-rows <out>.rows has the per-row sums.
// Not covered: bivariate HE, several matrices, REML.
//
// `--reml [--reml-trials T] [--reml-h2-start H] [--reml-cg-tol E] [--reml-cg-iters I] [--reml-tol X] [--reml-out F] [--reml-blup]` appended
// to a bayesMPI command line samples nothing either: the REML estimate of the SNP heritability of the same phenotype as --he, with
// [1 | covariates] as fixed effects, without ever forming the relationship matrix (run_reml): T sign probes seeded
// by --seed, a batched conjugate-gradient solve on the marker-dots and score pipelines, a secant search on log delta.
// <dir>/<name>.reml (or F) has the shape of GCTA's .hsq, then `key value` lines; --reml-blup adds <out>.blup with the marker effects.
// Not covered: several variance components, bivariate REML, LOCO, a likelihood value.  No parity with GCTA or BOLT is claimed.
//
// `--qc [--qc-out PREFIX] [--qc-maf X] [--qc-geno X] [--qc-mind X] [--qc-hwe P] [--qc-het-sd K]` appended to a bayesMPI command line samples
// nothing either: the quality control that comes before everything else, on the chain's rows.  Per marker, from the counts of
// hgibbs_marker_stats: allele frequency (.frq), call rate (.lmiss) and the exact Hardy-Weinberg test of hgibbs_hwe_exact (.hwe); per
// row, from ONE call of hgibbs_row_sums with seven tables: call rate (.imiss), homozygosity and F (.het) and GCTA's three inbreeding
// estimates (.ibc) over the autosomal markers with a finite sd (run_qc).  With thresholds, PREFIX.qc.exclude and
// PREFIX.qc.remove list what fails them; PREFIX defaults to <dir>/<name>.  Tab-separated; not byte parity with PLINK or GCTA.
//
// `--homozyg [--homozyg-window-snp W] [--homozyg-window-het H] [--homozyg-window-missing X] [--homozyg-window-threshold T] [--homozyg-snp S]
// [--homozyg-kb L] [--homozyg-density D] [--homozyg-gap G] [--homozyg-het H2] [--homozyg-out PREFIX]` appended to a bayesMPI command line
// samples nothing either: runs of homozygosity of the chain's rows over --qc's QC markers, PLINK 1.9's --homozyg scan restated in
// integers, as ONE call of hgibbs_roh (run_homozyg).  PREFIX.hom has one row per segment, PREFIX.hom.indiv one per
// row with F_ROH, PREFIX.hom.summary one per .bim marker; PREFIX defaults to <dir>/<name>.  Tab-separated; PLINK has not been run
// against it.  Not covered: --homozyg-group, windows above 64 markers, cM.
//
// `--epistasis [--epistasis-chisq T] [--epistasis-sets FILE] [--epistasis-gap KB] [--epistasis-out F]` appended to a bayesMPI command line
// samples nothing either: BOOST's exhaustive pairwise interaction scan of a case/control phenotype on the chain's rows (run_epistasis,
// DESIGN.md section 30).  ONE call of hgibbs_epi_scan screens every pair of markers by the Kirkwood bound on the device, hgibbs_epi_test
// fits the listed pairs on the host, and <dir>/<name>.epi.cc (or F) gets one row per pair with CHISQ >= T (default 30) and DF > 0.
// Covariates only drop rows.  Not covered: covariate adjustment, PLINK's allelic --fast-epistasis, case-only tests; neither PLINK nor
// BOOST has been run against it.
//
// `--sparse-dir D --sparse-basename B` reads the genotypes from hydra's ten sparse files D/B.{dim,sl?,ss?,si?} (? = 1, 2, m) instead of
// --bfile's .bed, for the chains and every mode above; --bfile is then optional for the chains (N = --number-individuals, the
// phenotype file is read line by line), and with it only .fam/.bim are taken from it.  `--bed-to-sparse --bfile X [--sparse-dir D
// --sparse-basename B]` writes those files from the whole X.bed and samples nothing.
//
// `--sumstats FILE [--sumstats-window W | --sumstats-window-kb KB] [--sumstats-n N]` on a bayesMPI command line samples the same
// mixture model from a table of per-marker effects (SNP A1 A2 BETA SE N, as --assoc writes them) and the LD band of the loaded panel
// (--bfile, or the sparse pair; --pheno is optional and only selects rows): .csv, .bet, .cpn and .acu in the chain's formats, so
// --predict-bfile and --pve read them.  Not covered: an LD band from a file or another cohort, covariates,
// BayesW, checkpoint and restart, several processes, GCTB's formats; parity with GCTB's SBayesR has not been run.
// `--sumstats-streams S` (1..1024) sweeps the independent LD blocks of the window (chromosomes, gaps wider than a kb window) at the
// same time in up to S streams, each from a generator of its own: the same posterior, another realisation.
// `--sumstats-chains R` (1..64) runs R chains from the seeds --seed + r on the one band, one launch per iteration for all of them
// (DESIGN.md section 33): chain 0 writes the files of the run without the option, chain r >= 1 writes <name>.c<r>.{csv,bet,cpn,acu},
// the files of the run with --seed raised by r; <name>.rhat holds split-R^ and the effective sample size of the hyper-parameters.
// `--sumstats-post [--sumstats-post-all] [--sumstats-post-only] [--sumstats-post-out F]` writes <name>.post (or F), one row per .bim
// marker: posterior mean and sd of the effect, PIP, component shares and split-R^ over the chains, accumulated on the device from the
// thinned records at or after --burn-in (-all: every iteration from there; -only: no .bet, .cpn, .acu at all).
// `--sumstats-cs [--sumstats-cs-r2 T] [--sumstats-cs-alpha A] [--sumstats-cs-pep P] [--sumstats-cs-lead L] [--sumstats-cs-max-size K]
// [--sumstats-cs-out F]` writes <name>.cs (or F): local credible sets from the inclusion history of the thinned records at or after
// --burn-in, one bit per marker and record kept on the device.  `--cs [--cs-chains R] [--cs-window-kb KB |
// --cs-window-snps W] [--cs-r2 T] [--cs-alpha A] [--cs-pep P] [--cs-lead L] [--cs-max-size K] [--cs-out F]`, appended to a bayesMPI
// command line, samples nothing and writes the same table from a finished chain's <name>.bet (and <name>.c<r>.bet).  Not covered:
// GCTB's rule for overlapping sets and its .lcs layout, the share of heritability per set; GCTB has not been run against it.
//
// Not reproduced (out of scope for the hot path): the mixed
// in-memory representation (--threshold-fnz), --sparse-sync/--bed-sync, --check-RAM,
// marker-block files, bayesFH, marker-sharded MPI, the .lst/tarball.
// Multi-GPU: one process per GPU (RANK/WORLD_SIZE/LOCAL_RANK in the
// environment, as torchrun/mpirun export them); individuals are sharded and the
// ncclUniqueId travels through a file in --mcmc-out-dir.
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <initializer_list>
#include <iostream>
#include <limits>
#include <map>
#include <optional>
#include <sstream>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/hgibbs.h"

namespace {

// the sub-options the two credible-set routes share, as given (empty: not given; checked before the device)
struct CsStrings {
    std::string r2, alpha, pep, lead, maxSize, out; // -r2 T, -alpha A, -pep P, -lead L, -max-size K, -out F
};

struct Options { // src/options.hpp:20-138 (subset that reaches bayesMPI)
    std::string bayesType, analysisType = "Bayes";
    std::string bedFile, phenotypeFile, mcmcOutDir, mcmcOutNam, groupIndexFile, groupMixtureFile, covariatesFile;
    bool covariates = false;
    unsigned chainLength = 10000, burnin = 5000, thin = 5, save = 10;
    unsigned seed = 0;
    bool seedGiven = false;
    unsigned numberMarkers = 0, numberIndividuals = 0;
    int shuffleMarkers = 1, syncRate = 1;
    std::vector<double> S{0.01, 0.001, 0.0001};
    bool readFromBedFile = false;
    bool restart = false, useXfilesInRestart = true; // options.hpp:33-34
    std::string failureFile, quad_points;            // options.hpp:56-58 (bayesWMPI)
    std::string predictBfile, predictOut;            // --predict-bfile / --predict-out: score a target cohort (this build's, not hydra's)
    bool predictDryRun = false;                      // --predict-dry-run: every check and the match report, then stop before the device
    long long ldWindow = 0;                          // --ld-window W: windowed LD of the training markers
    double ldWindowKb = -1.0, ldWindowR2 = 0.2;      // --ld-window-kb (-1: no bp limit), --ld-window-r2
    bool ldGiven = false, ldKbGiven = false, ldR2Given = false, ldBin = false;
    std::string ldOut;                               // --ld-out
    bool assoc = false, assocNoLoco = false;         // --assoc: per-marker association tests; --assoc-no-loco: without LOCO offsets
    std::string assocOut;                            // --assoc-out
    bool assocLogistic = false;                      // --assoc-logistic: the logistic score test of a case/control phenotype
    bool assocSpa = false, assocSpaSdGiven = false;  // --assoc-spa: saddlepoint p-values for the markers whose score is beyond --assoc-spa-sd SD
    std::string assocSpaSd = "2";                    // --assoc-spa-sd
    bool assocFirth = false, assocFirthPGiven = false; // --assoc-firth: Firth's penalised fit for the markers whose score-test P is at most --assoc-firth-p
    std::string assocFirthP = "0.05";                // --assoc-firth-p
    std::string assocSets, assocSetOut;              // --assoc-sets FILE: burden and SKAT of the file's marker sets; --assoc-set-out
    std::string assocSetA = "1", assocSetB = "25", assocSetMaf = "0.5"; // --assoc-set-beta A B, --assoc-set-maf X as given
    bool assocSetBetaGiven = false, assocSetMafGiven = false;
    bool king = false, kingCutoffGiven = false;      // --king: KING-robust kinship of the chain's rows; --king-cutoff given
    std::string kingCutoff = "0.0442", kingOut;      // --king-cutoff T (checked before the device), --king-out
    bool pca = false, pcaLoadings = false, pcaItersGiven = false, pcaTolGiven = false, pcaOutGiven = false; // --pca K; which --pca-* were given
    std::string pcaK, pcaIters, pcaTol, pcaOut;      // --pca K, --pca-iters P, --pca-tol T as given (checked before the device), --pca-out
    bool pve = false, pveKbGiven = false, pveSnpsGiven = false, pveGroups = false, pveThresholdGiven = false, pveBin = false; // --pve; which --pve-* were given
    std::string pveKb, pveSnps, pveSets, pveThreshold, pveOut; // --pve-window-kb KB, --pve-window-snps W, --pve-threshold T as given, --pve-sets, --pve-out
    bool grm = false, grmSparseGiven = false;        // --grm: genomic relationship matrix of the chain's rows; --grm-sparse given
    std::string grmOut, grmSparse;                   // --grm-out PREFIX, --grm-sparse T as given (checked before the device)
    bool he = false, heRows = false;                 // --he: Haseman-Elston regression on the chain's rows; --he-rows: the per-row sums too
    std::string heOut;                               // --he-out F
    bool reml = false, remlBlup = false;             // --reml: REML heritability without the relationship matrix; --reml-blup: the marker effects too
    std::string remlTrials, remlH2, remlCgTol, remlCgIters, remlTol, remlOut; // --reml-trials T, --reml-h2-start H, --reml-cg-tol E, --reml-cg-iters I, --reml-tol X as given, --reml-out F
    bool qc = false, qcMafGiven = false, qcGenoGiven = false, qcMindGiven = false, qcHweGiven = false, qcHetSdGiven = false; // --qc; which thresholds were given
    bool epistasis = false; // --epistasis: BOOST's pairwise interaction scan of a case/control phenotype (run_epistasis)
    std::string epiChisq, epiSets, epiGap, epiOut; // --epistasis-chisq T, --epistasis-gap KB as given (checked before the device), --epistasis-sets, --epistasis-out F
    bool homozyg = false; // --homozyg: runs of homozygosity of the chain's rows (run_homozyg)
    // --homozyg-window-snp W, -window-het H, -window-missing X, -window-threshold T, -snp S, -kb L, -density D, -gap G, -het H2 as given
    // (empty: PLINK 1.9's default; checked before the device), --homozyg-out PREFIX
    std::string hzWindow, hzWindowHet, hzWindowMissing, hzThreshold, hzSnp, hzKb, hzDensity, hzGap, hzHet, hzOut;
    std::string qcOut, qcMaf, qcGeno, qcMind, qcHwe, qcHetSd; // --qc-out PREFIX; --qc-maf X, --qc-geno X, --qc-mind X, --qc-hwe P, --qc-het-sd K as given (checked before the device)
    bool ldScore = false, ldScoreKbGiven = false, ldScoreSnpsGiven = false, ldScoreGroups = false, ldScoreRaw = false; // --ld-score; which --ld-score-* were given
    std::string ldScoreKb, ldScoreSnps, ldScoreSets, ldScoreOut; // --ld-score-kb KB, --ld-score-snps W as given (checked before the device), --ld-score-sets, --ld-score-out PREFIX
    bool clump = false, clumpKbGiven = false, clumpSnpsGiven = false; // --clump FILE; which window option was given
    std::string clumpFile, clumpP1, clumpP2, clumpR2, clumpKb, clumpSnps, clumpSnpField, clumpField, clumpOut; // --clump-* as given (checked before the device; empty: not given)
    bool ldPrune = false, ldPruneKbGiven = false, ldPruneSnpsGiven = false; // --ld-prune T; which window option was given
    std::string ldPruneT, ldPruneKb, ldPruneSnps, ldPruneOut; // --ld-prune T, --ld-prune-kb KB, --ld-prune-snps W as given, --ld-prune-out PREFIX
    std::string sparseDir, sparseBsn;                // --sparse-dir D --sparse-basename B: hydra's sparse genotype files D/B.*
    bool bedToSparse = false, preferBed = false;     // --bed-to-sparse: write them from --bfile; --read-from-bed-file: read the BED though the pair is given
    bool blocksPerRankGiven = false;                 // --blocks-per-rank n: hydra's marker-sharded layout, no meaning here
    bool sumstats = false, sumstatsWindowGiven = false, sumstatsKbGiven = false, sumstatsNGiven = false; // --sumstats FILE; which --sumstats-* were given
    std::string sumstatsFile, sumstatsWindow, sumstatsKb, sumstatsN; // --sumstats-window W, --sumstats-window-kb KB, --sumstats-n N as given (checked before the device)
    bool sumstatsStreamsGiven = false; // --sumstats-streams S: independent LD blocks in up to S parallel streams
    std::string sumstatsStreams;
    bool sumstatsChainsGiven = false; // --sumstats-chains R: R chains from the seeds --seed + r on one band, with a .rhat table
    std::string sumstatsChains;
    bool sumstatsPost = false, sumstatsPostAll = false, sumstatsPostOnly = false; // --sumstats-post: the per-marker posterior table
    std::string sumstatsPostOut; // --sumstats-post-out F
    bool sumstatsCs = false; // --sumstats-cs: local credible sets from the chains' inclusion history on the device
    CsStrings ssCs;          // --sumstats-cs-* as given
    bool cs = false, csKbGiven = false, csSnpsGiven = false; // --cs: the same sets from a finished chain's .bet; which window option was given
    std::string csChains, csKb, csSnps; // --cs-chains R, --cs-window-kb KB, --cs-window-snps W as given
    CsStrings csArgs;                   // --cs-r2 .. --cs-out as given
    bool saveGiven = false, ignoreXfilesGiven = false; // --save, --ignore-xfiles on the command line (--sumstats takes no checkpoint option)
    int batch = 0, cpg = 0; // tuning knobs of this build (not hydra's)
};

[[noreturn]] void fatal(const std::string& m)
{
    std::fprintf(stderr, "\n%s\n", m.c_str());
    std::exit(1);
}

// Gadget::Tokenizer::getTokens, src/gadgets.cpp:12-22
std::vector<std::string> tokens(const std::string& str, const std::string& sep)
{
    std::vector<std::string> out;
    std::string::size_type b = str.find_first_not_of(sep);
    while (b != std::string::npos) {
        std::string::size_type e = str.find_first_of(sep, b);
        if (e == std::string::npos) e = str.length();
        out.push_back(str.substr(b, e - b));
        b = str.find_first_not_of(sep, e);
    }
    return out;
}

// Options::readFile, src/options.cpp:335-397: "key value" pairs; a key that starts with // or # skips its value token; an
// unknown key is an error.  mcmcOut is the output prefix (directory/name); the bed file named here is read as --bfile would.
void read_option_file(const std::string& file, Options& o)
{
    std::ifstream in(file.c_str());
    if (!in) fatal("Error: can not open the file [" + file + "] to read.");
    std::string key, value;
    while (in >> key >> value) {
        if (key == "bedFile") {
            o.bedFile = value;
            o.readFromBedFile = true;
        } else if (key == "phenotypeFile") o.phenotypeFile = value;
        else if (key == "analysisType") o.analysisType = value;
        else if (key == "bayesType") o.bayesType = value;
        else if (key == "mcmcOut") {
            const std::string::size_type cut = value.find_last_of('/');
            o.mcmcOutDir = cut == std::string::npos ? std::string(".") : (cut == 0 ? std::string("/") : value.substr(0, cut));
            o.mcmcOutNam = cut == std::string::npos ? value : value.substr(cut + 1);
        } else if (key == "shuffleMarkers") o.shuffleMarkers = std::stoi(value);
        else if (key == "syncRate") o.syncRate = std::stoi(value);
        else if (key == "blocksPerRank") (void)std::stoi(value); // hydra's marker-sharded MPI layout: no meaning here (individuals shard)
        else if (key == "numberMarkers") o.numberMarkers = (unsigned)std::stoi(value);
        else if (key == "numberIndividuals") o.numberIndividuals = (unsigned)std::stoi(value);
        else if (key == "chainLength") o.chainLength = (unsigned)std::stoi(value);
        else if (key == "burnin") o.burnin = (unsigned)std::stoi(value);
        else if (key == "seed") {
            o.seed = (unsigned)std::stoi(value);
            o.seedGiven = true;
        } else if (key == "thin") o.thin = (unsigned)std::stoi(value);
        else if (key == "save") o.save = (unsigned)std::stoi(value);
        else if (key == "S") {
            o.S.clear();
            // (the reference reads these through stof, src/options.cpp:384: the option file's 0.0001 is 9.99999974737875e-05 in the chain,
            // unlike --S on the command line, which goes through stod)
            for (const std::string& t : tokens(value, " ,")) o.S.push_back((double)std::stof(t));
        } else if (key.substr(0, 2) == "//" || key.substr(0, 1) == "#") {
            continue;
        } else {
            fatal("\nError: invalid option " + key + " " + value + "\n");
        }
    }
}

Options parse(int argc, const char* argv[])
{
    Options o;
    auto need = [&](int& i) -> const char* {
        if (i + 1 >= argc) fatal(std::string("missing value after ") + argv[i]);
        return argv[++i];
    };
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--inp-file") { // options.cpp:8-11: the file replaces the rest of the command line
            read_option_file(need(i), o);
            if (!o.seedGiven) o.seed = (unsigned)std::time(nullptr);
            return o;
        }
        if (a == "--mpibayes" || a == "--bayesType") { // --bayesType: alias (it is the option-file key, options.cpp:353)
            o.analysisType = "RAM";
            o.bayesType = need(i);
        } else if (a == "--bfile") {
            o.readFromBedFile = true;
            o.bedFile = need(i);
        } else if (a == "--pheno") {
            o.phenotypeFile = tokens(need(i), ",").at(0);
        } else if (a == "--mcmc-out-dir") o.mcmcOutDir = need(i);
        else if (a == "--mcmc-out-name") o.mcmcOutNam = need(i);
        else if (a == "--shuf-mark") o.shuffleMarkers = std::atoi(need(i));
        else if (a == "--sync-rate") o.syncRate = std::atoi(need(i));
        else if (a == "--number-markers") o.numberMarkers = (unsigned)std::atoi(need(i));
        else if (a == "--number-individuals") o.numberIndividuals = (unsigned)std::atoi(need(i));
        else if (a == "--chain-length") o.chainLength = (unsigned)std::atoi(need(i));
        else if (a == "--burn-in") o.burnin = (unsigned)std::atoi(need(i));
        else if (a == "--seed") {
            o.seed = (unsigned)std::atoi(need(i));
            o.seedGiven = true;
        } else if (a == "--thin") o.thin = (unsigned)std::atoi(need(i));
        else if (a == "--save") {
            o.save = (unsigned)std::atoi(need(i));
            o.saveGiven = true;
        }
        else if (a == "--S") {
            o.S.clear();
            for (const std::string& t : tokens(need(i), " ,")) o.S.push_back(std::stod(t));
        } else if (a == "--groupIndexFile") o.groupIndexFile = need(i);
        else if (a == "--groupMixtureFile") o.groupMixtureFile = need(i);
        else if (a == "--batch") o.batch = std::atoi(need(i));
        else if (a == "--cols-per-group") o.cpg = std::atoi(need(i));
        else if (a == "--covariates") {
            o.covariates = true;
            o.covariatesFile = need(i);
        } else if (a == "--failure") o.failureFile = need(i);    // options.cpp:183-186
        else if (a == "--quad_points") o.quad_points = need(i); // options.cpp:188-191
        else if (a == "--restart") o.restart = true;          // options.cpp:63-65
        else if (a == "--ignore-xfiles") {                              // options.cpp:67-69
            o.useXfilesInRestart = false;
            o.ignoreXfilesGiven = true;
        } else if (a == "--sumstats") {
            o.sumstatsFile = need(i);
            o.sumstats = true;
        } else if (a == "--sumstats-window") {
            o.sumstatsWindow = need(i);
            o.sumstatsWindowGiven = true;
        } else if (a == "--sumstats-window-kb") {
            o.sumstatsKb = need(i);
            o.sumstatsKbGiven = true;
        } else if (a == "--sumstats-streams") {
            o.sumstatsStreams = need(i);
            o.sumstatsStreamsGiven = true;
        } else if (a == "--sumstats-chains") {
            o.sumstatsChains = need(i);
            o.sumstatsChainsGiven = true;
        } else if (a == "--sumstats-post") {
            o.sumstatsPost = true;
        } else if (a == "--sumstats-post-all") {
            o.sumstatsPostAll = true;
        } else if (a == "--sumstats-post-only") {
            o.sumstatsPostOnly = true;
        } else if (a == "--sumstats-post-out") {
            o.sumstatsPostOut = need(i);
        } else if (a == "--sumstats-n") {
            o.sumstatsN = need(i);
            o.sumstatsNGiven = true;
        } else if (a == "--sumstats-cs") o.sumstatsCs = true;
        else if (a == "--sumstats-cs-r2") o.ssCs.r2 = need(i);
        else if (a == "--sumstats-cs-alpha") o.ssCs.alpha = need(i);
        else if (a == "--sumstats-cs-pep") o.ssCs.pep = need(i);
        else if (a == "--sumstats-cs-lead") o.ssCs.lead = need(i);
        else if (a == "--sumstats-cs-max-size") o.ssCs.maxSize = need(i);
        else if (a == "--sumstats-cs-out") o.ssCs.out = need(i);
        else if (a == "--cs") o.cs = true;
        else if (a == "--cs-chains") o.csChains = need(i);
        else if (a == "--cs-window-kb") {
            o.csKb = need(i);
            o.csKbGiven = true;
        } else if (a == "--cs-window-snps") {
            o.csSnps = need(i);
            o.csSnpsGiven = true;
        } else if (a == "--cs-r2") o.csArgs.r2 = need(i);
        else if (a == "--cs-alpha") o.csArgs.alpha = need(i);
        else if (a == "--cs-pep") o.csArgs.pep = need(i);
        else if (a == "--cs-lead") o.csArgs.lead = need(i);
        else if (a == "--cs-max-size") o.csArgs.maxSize = need(i);
        else if (a == "--cs-out") o.csArgs.out = need(i);
        else if (a == "--predict-bfile") o.predictBfile = need(i);
        else if (a == "--predict-out") o.predictOut = need(i);
        else if (a == "--predict-dry-run") o.predictDryRun = true;
        else if (a == "--ld-window") {
            o.ldWindow = std::atoll(need(i));
            o.ldGiven = true;
        }
        else if (a == "--ld-window-kb") {
            o.ldWindowKb = std::atof(need(i));
            o.ldKbGiven = true;
        } else if (a == "--ld-window-r2") {
            o.ldWindowR2 = std::atof(need(i));
            o.ldR2Given = true;
        } else if (a == "--ld-out") o.ldOut = need(i);
        else if (a == "--ld-bin") o.ldBin = true;
        else if (a == "--assoc") o.assoc = true;
        else if (a == "--assoc-no-loco") o.assocNoLoco = true;
        else if (a == "--assoc-out") o.assocOut = need(i);
        else if (a == "--assoc-logistic") o.assocLogistic = true;
        else if (a == "--assoc-spa") o.assocSpa = true;
        else if (a == "--assoc-spa-sd") { o.assocSpaSd = need(i); o.assocSpaSdGiven = true; }
        else if (a == "--assoc-firth") o.assocFirth = true;
        else if (a == "--assoc-firth-p") { o.assocFirthP = need(i); o.assocFirthPGiven = true; }
        else if (a == "--assoc-sets") o.assocSets = need(i);
        else if (a == "--assoc-set-beta") { o.assocSetA = need(i); o.assocSetB = need(i); o.assocSetBetaGiven = true; }
        else if (a == "--assoc-set-maf") { o.assocSetMaf = need(i); o.assocSetMafGiven = true; }
        else if (a == "--assoc-set-out") o.assocSetOut = need(i);
        else if (a == "--king") o.king = true;
        else if (a == "--king-cutoff") {
            o.kingCutoff = need(i);
            o.kingCutoffGiven = true;
        } else if (a == "--king-out") o.kingOut = need(i);
        else if (a == "--pca") {
            o.pcaK = need(i);
            o.pca = true;
        } else if (a == "--pca-iters") {
            o.pcaIters = need(i);
            o.pcaItersGiven = true;
        } else if (a == "--pca-tol") {
            o.pcaTol = need(i);
            o.pcaTolGiven = true;
        } else if (a == "--pca-out") {
            o.pcaOut = need(i);
            o.pcaOutGiven = true;
        } else if (a == "--pca-loadings") o.pcaLoadings = true;
        else if (a == "--pve") o.pve = true;
        else if (a == "--pve-window-kb") {
            o.pveKb = need(i);
            o.pveKbGiven = true;
        } else if (a == "--pve-window-snps") {
            o.pveSnps = need(i);
            o.pveSnpsGiven = true;
        } else if (a == "--pve-sets") o.pveSets = need(i);
        else if (a == "--pve-groups") o.pveGroups = true;
        else if (a == "--pve-threshold") {
            o.pveThreshold = need(i);
            o.pveThresholdGiven = true;
        } else if (a == "--pve-out") o.pveOut = need(i);
        else if (a == "--pve-bin") o.pveBin = true;
        else if (a == "--grm") o.grm = true;
        else if (a == "--grm-out") o.grmOut = need(i);
        else if (a == "--he") o.he = true;
        else if (a == "--he-out") o.heOut = need(i);
        else if (a == "--he-rows") o.heRows = true;
        else if (a == "--reml") o.reml = true;
        else if (a == "--reml-trials") o.remlTrials = need(i);
        else if (a == "--reml-h2-start") o.remlH2 = need(i);
        else if (a == "--reml-cg-tol") o.remlCgTol = need(i);
        else if (a == "--reml-cg-iters") o.remlCgIters = need(i);
        else if (a == "--reml-tol") o.remlTol = need(i);
        else if (a == "--reml-out") o.remlOut = need(i);
        else if (a == "--reml-blup") o.remlBlup = true;
        else if (a == "--epistasis") o.epistasis = true;
        else if (a == "--epistasis-chisq") o.epiChisq = need(i);
        else if (a == "--epistasis-sets") o.epiSets = need(i);
        else if (a == "--epistasis-gap") o.epiGap = need(i);
        else if (a == "--epistasis-out") o.epiOut = need(i);
        else if (a == "--homozyg") o.homozyg = true;
        else if (a == "--homozyg-window-snp") o.hzWindow = need(i);
        else if (a == "--homozyg-window-het") o.hzWindowHet = need(i);
        else if (a == "--homozyg-window-missing") o.hzWindowMissing = need(i);
        else if (a == "--homozyg-window-threshold") o.hzThreshold = need(i);
        else if (a == "--homozyg-snp") o.hzSnp = need(i);
        else if (a == "--homozyg-kb") o.hzKb = need(i);
        else if (a == "--homozyg-density") o.hzDensity = need(i);
        else if (a == "--homozyg-gap") o.hzGap = need(i);
        else if (a == "--homozyg-het") o.hzHet = need(i);
        else if (a == "--homozyg-out") o.hzOut = need(i);
        else if (a == "--qc") o.qc = true;
        else if (a == "--qc-out") o.qcOut = need(i);
        else if (a == "--qc-maf") {
            o.qcMaf = need(i);
            o.qcMafGiven = true;
        } else if (a == "--qc-geno") {
            o.qcGeno = need(i);
            o.qcGenoGiven = true;
        } else if (a == "--qc-mind") {
            o.qcMind = need(i);
            o.qcMindGiven = true;
        } else if (a == "--qc-hwe") {
            o.qcHwe = need(i);
            o.qcHweGiven = true;
        } else if (a == "--qc-het-sd") {
            o.qcHetSd = need(i);
            o.qcHetSdGiven = true;
        }
        else if (a == "--grm-sparse") {
            o.grmSparse = need(i);
            o.grmSparseGiven = true;
        } else if (a == "--ld-score") o.ldScore = true;
        else if (a == "--ld-score-kb") {
            o.ldScoreKb = need(i);
            o.ldScoreKbGiven = true;
        } else if (a == "--ld-score-snps") {
            o.ldScoreSnps = need(i);
            o.ldScoreSnpsGiven = true;
        } else if (a == "--ld-score-sets") o.ldScoreSets = need(i);
        else if (a == "--ld-score-groups") o.ldScoreGroups = true;
        else if (a == "--ld-score-raw") o.ldScoreRaw = true;
        else if (a == "--ld-score-out") o.ldScoreOut = need(i);
        else if (a == "--clump") {
            o.clumpFile = need(i);
            o.clump = true;
        } else if (a == "--clump-p1") o.clumpP1 = need(i);
        else if (a == "--clump-p2") o.clumpP2 = need(i);
        else if (a == "--clump-r2") o.clumpR2 = need(i);
        else if (a == "--clump-kb") {
            o.clumpKb = need(i);
            o.clumpKbGiven = true;
        } else if (a == "--clump-snps") {
            o.clumpSnps = need(i);
            o.clumpSnpsGiven = true;
        } else if (a == "--clump-snp-field") o.clumpSnpField = need(i);
        else if (a == "--clump-field") o.clumpField = need(i);
        else if (a == "--clump-out") o.clumpOut = need(i);
        else if (a == "--ld-prune") {
            o.ldPruneT = need(i);
            o.ldPrune = true;
        } else if (a == "--ld-prune-kb") {
            o.ldPruneKb = need(i);
            o.ldPruneKbGiven = true;
        } else if (a == "--ld-prune-snps") {
            o.ldPruneSnps = need(i);
            o.ldPruneSnpsGiven = true;
        } else if (a == "--ld-prune-out") o.ldPruneOut = need(i);
        else if (a == "--sparse-dir") o.sparseDir = need(i);
        else if (a == "--sparse-basename") o.sparseBsn = need(i);
        else if (a == "--bed-to-sparse") o.bedToSparse = true;
        else if (a == "--read-from-bed-file") o.preferBed = true;
        else if (a == "--blocks-per-rank") {
            (void)need(i);
            o.blocksPerRankGiven = true;
        } else if (a == "--sparse-sync" || a == "--bed-sync")
            fatal("FATAL  : option " + a + " belongs to a part of hydra this build does not reproduce (SURVEY.md section 2)");
        else
            fatal("\nError: invalid option \"" + a + "\".\n"); // options.cpp:292-295
    }
    if (!o.seedGiven) o.seed = (unsigned)std::time(nullptr); // options.hpp:105
    if (o.sparseDir.empty() != o.sparseBsn.empty())          // options.cpp:328-331
        fatal("FATAL  : --sparse-dir and --sparse-basename must either be both set or unset (this build does not reproduce a default for one of them)");
    if (o.analysisType == "RAM" && !o.bedToSparse) {         // options.cpp:303-326
        if (o.mcmcOutDir.empty()) fatal("FATAL  : --mcmc-out-dir is mandatory with --mpibayes");
        if (o.mcmcOutNam.empty()) fatal("FATAL  : --mcmc-out-name is mandatory with --mpibayes");
    }
    return o;
}

// ---- what every path of the CLI does with its files, once -------------------
// an option's argument as an integer, resp. a number: false unless the whole argument is one
bool whole_int(const std::string& t, long& v)
{
    const char* s = t.c_str();
    char* end = nullptr;
    v = std::strtol(s, &end, 10);
    return end != s && *end == 0;
}

bool whole_num(const std::string& t, double& v)
{
    const char* s = t.c_str();
    char* end = nullptr;
    v = std::strtod(s, &end);
    return end != s && *end == 0;
}

// FID and IID of the rows of a .fam, at most `limit` of them; with `keep`, only of the rows it marks
struct FamIds {
    std::vector<std::string> fid, iid;
};

FamIds read_fam_ids(const std::string& path, size_t limit, const std::vector<uint8_t>* keep)
{
    std::ifstream in(path);
    if (!in) fatal("Error: can not open the file [" + path + "] to read.");
    FamIds ids;
    std::string f, i, dad, mom, sex, phen;
    for (size_t r = 0; r < limit && (in >> f >> i >> dad >> mom >> sex >> phen); ++r) // data.cpp:1454
        if (!keep || (*keep)[r]) {
            ids.fid.push_back(f);
            ids.iid.push_back(i);
        }
    return ids;
}

// the genotypes of <prefix>.bed after its magic: M x ceil(numInds / 4) bytes
std::vector<uint8_t> read_bed(const std::string& prefix, size_t numInds, size_t M)
{
    std::ifstream in(prefix + ".bed", std::ios::binary);
    if (!in) fatal("Error: can not open the file [" + prefix + ".bed] to read.");
    unsigned char magic[3];
    in.read((char*)magic, 3);
    if (!in || magic[0] != 0x6c || magic[1] != 0x1b || magic[2] != 0x01) fatal("FATAL  : " + prefix + ".bed is not a SNP-major PLINK bed");
    std::vector<uint8_t> bed(M * ((numInds + 3) / 4));
    in.read((char*)bed.data(), (std::streamsize)bed.size());
    if ((size_t)in.gcount() != bed.size()) fatal("FATAL  : " + prefix + ".bed is shorter than M x ceil(N/4)");
    return bed;
}

// --mcmc-out-dir, made when it is not there (the caller asks when an output goes to its default path)
void make_out_dir(const Options& o)
{
    struct stat sb;
    if (stat(o.mcmcOutDir.c_str(), &sb) != 0 && std::system(("mkdir -p " + o.mcmcOutDir).c_str()) != 0) fatal("FATAL  : can not create --mcmc-out-dir");
}

FILE* open_out(const std::string& p, const char* mode)
{
    FILE* f = std::fopen(p.c_str(), mode);
    if (!f) fatal("FATAL  : can not create " + p);
    return f;
}

void close_out(FILE* f, const std::string& p)
{
    if (std::fclose(f) != 0) fatal("FATAL  : short write on " + p);
}

size_t count_fam(const std::string& path, std::vector<std::string>* ids)
{
    const FamIds fam = read_fam_ids(path, (size_t)-1, nullptr);
    std::map<std::string, int> seen;
    for (size_t r = 0; r < fam.fid.size(); ++r) {
        const std::string id = fam.fid[r] + ":" + fam.iid[r];
        if (!seen.emplace(id, 1).second) fatal("Error: Duplicate individual ID found: \"" + fam.fid[r] + "\t" + fam.iid[r] + "\".");
        if (ids) ids->push_back(id);
    }
    return fam.fid.size();
}

size_t count_bim(const std::string& path)
{
    std::ifstream in(path);
    if (!in) fatal("Error: can not open the file [" + path + "] to read.");
    std::string id, a1, a2;
    unsigned chr, pos;
    float gpos;
    size_t n = 0;
    while (in >> chr >> id >> gpos >> pos >> a1 >> a2) ++n; // data.cpp:1484
    return n;
}

// Data::readPhenotypeFile(phenFile), src/data.cpp:1840-1882: lines whose FID:IID
// is in the .fam are taken in FILE order; "NA" marks a dropped individual.
void read_phen(const std::string& path, const std::vector<std::string>& fam_ids, std::vector<double>& y,
               std::vector<uint8_t>& keep)
{
    std::ifstream in(path);
    if (!in) fatal("Error: can not open the phenotype file [" + path + "] to read.");
    std::map<std::string, int> idx;
    for (size_t i = 0; i < fam_ids.size(); ++i) idx[fam_ids[i]] = (int)i;
    keep.assign(fam_ids.size(), 1);
    y.clear();
    std::string line;
    size_t lineno = 0;
    while (std::getline(in, line)) {
        std::vector<std::string> col = tokens(line, " \t");
        if (col.size() < 3) continue;
        if (!idx.count(col[0] + ":" + col[1])) continue;
        if (lineno >= keep.size()) break;
        if (col[2] != "NA") y.push_back(std::atof(col[2].c_str()));
        else keep[lineno] = 0; // NAsInds.push_back(line)
        ++lineno;
    }
    if (lineno != fam_ids.size()) fatal("FATAL  : phenotype file covers " + std::to_string(lineno) + " of " + std::to_string(fam_ids.size()) + " individuals");
}

// Data::readPhenCovFiles, src/data.cpp:1615-1673: .phen and .cov are read line by line in
// lockstep (no .fam lookup); an individual is dropped if its phenotype or any covariate is NA.
void read_phen_cov(const std::string& phen, const std::string& cov, size_t numInds, std::vector<double>& y,
                   std::vector<uint8_t>& keep, std::vector<double>& X, int& C)
{
    std::ifstream inp(phen), inc(cov);
    if (!inp) fatal("Error: can not open the phenotype file [" + phen + "] to read.");
    if (!inc) fatal("Error: can not open the covariates file [" + cov + "] to read.");
    keep.assign(numInds, 1);
    y.clear();
    X.clear();
    std::string lp, lc;
    size_t line = 0;
    while (std::getline(inp, lp)) {
        if (!std::getline(inc, lc)) fatal("FATAL  : covariates file is shorter than the phenotype file");
        if (line >= numInds) break;
        std::vector<std::string> cp = tokens(lp, " \t"), cc = tokens(lc, " \t");
        if (cp.size() < 3) continue;
        bool naC = false;
        for (size_t i = 2; i < cc.size(); ++i)
            if (cc[i] == "NA") naC = true;
        if (cp[2] != "NA" && !naC) {
            y.push_back(std::atof(cp[2].c_str()));
            for (size_t i = 2; i < cc.size(); ++i) X.push_back(std::stod(cc[i]));
        } else {
            keep[line] = 0;
        }
        ++line;
    }
    if (line != numInds) fatal("FATAL  : phenotype/covariates files cover " + std::to_string(line) + " of " + std::to_string(numInds) + " individuals");
    C = y.empty() ? 0 : (int)(X.size() / y.size());
    std::printf("numFixedEffect = %d\n", C);
}

std::vector<int32_t> read_groups(const std::string& path) // data.cpp:1940-1958
{
    std::ifstream in(path);
    if (!in) fatal("Error: can not open the group file [" + path + "] to read. Use the --groupIndexFile option!");
    std::vector<int32_t> g;
    int v;
    while (in >> v) g.push_back(v);
    return g;
}

std::vector<std::vector<double>> read_mS(const std::string& path) // data.cpp:1963-2004
{
    std::ifstream in(path);
    if (!in) fatal("Error: can not open the mixture file [" + path + "] to read. Use the --groupMixtureFile option!");
    std::string text((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    std::vector<std::string> rows = tokens(text, ";");
    std::vector<std::vector<double>> mS;
    size_t ncomp = 0;
    for (const std::string& r : rows) {
        std::vector<std::string> t = tokens(r, ",");
        // a trailing newline after the last ';' group is not a group
        bool blank = true;
        for (char ch : r)
            if (!std::isspace((unsigned char)ch)) blank = false;
        if (blank) continue;
        if (ncomp == 0) ncomp = t.size();
        if (t.size() != ncomp) fatal("FATAL  : all group mixture should have the same number of components");
        std::vector<double> row{0.0};
        for (const std::string& x : t) {
            const double mix = std::stod(x);
            if (mix <= 0.0) fatal("FATAL  : mixture value can only be strictly positive");
            row.push_back(mix);
        }
        mS.push_back(row);
    }
    return mS;
}

void hg_check(int rc, const char* what)
{
    if (rc) fatal(std::string("FATAL  : ") + what + ": " + hgibbs_last_error());
}

void pwrite_at(FILE* f, long off, const void* p, size_t n)
{
    if (std::fseek(f, off, SEEK_SET) != 0 || std::fwrite(p, 1, n, f) != n) fatal("FATAL  : short write on an output file");
}

double now_s()
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// ---- hydra's sparse genotype files --------------------------------------------------------------------------
// <dir>/<basename>.dim, the text "N M", and per class c in {1, 2, m} (genotype 1, genotype 2, missing call): .sl<c> and .ss<c>, M uint64
// each (a marker's entries, the absolute position of its first entry), and .si<c>, the uint32 row indices (layout restated from
// src/BayesRRm.cpp:437-770 and src/data.cpp:1072-1106, 1224-1290)
const char* const SP_CLASS[3] = {"1", "2", "m"};

struct SparseSource {
    bool on = false;                    // the genotypes come from the sparse files, not from --bfile's .bed
    std::string prefix;                 // <dir>/<basename>
    std::vector<uint64_t> ss[3], sl[3]; // the first --number-markers entries of the six files
};
SparseSource g_sparse;

bool use_sparse(const Options& o)
{
    return !o.sparseDir.empty() && !o.preferBed;
}

uint64_t readable_size(const std::string& p)
{
    struct stat sb;
    FILE* f = std::fopen(p.c_str(), "rb");
    if (!f || stat(p.c_str(), &sb) != 0 || !S_ISREG(sb.st_mode)) fatal("Error: can not open the file [" + p + "] to read.");
    std::fclose(f);
    return (uint64_t)sb.st_size;
}

// Every check of the sparse files, before any device is created; each refusal names the file and the fact.
void open_sparse(const Options& opt, size_t numInds, unsigned M)
{
    SparseSource& s = g_sparse;
    s.prefix = opt.sparseDir + "/" + opt.sparseBsn;
    const std::string dim = s.prefix + ".dim";
    (void)readable_size(dim);
    std::ifstream in(dim);
    long long n = -1, m = -1;
    if (!(in >> n >> m) || n <= 0 || m <= 0) fatal("FATAL  : " + dim + " does not parse as \"N M\"");
    if ((unsigned long long)n != numInds)
        fatal("FATAL  : " + dim + " says N = " + std::to_string(n) + ", --number-individuals says " + std::to_string(numInds));
    if ((unsigned long long)m < M) fatal("FATAL  : " + dim + " says M = " + std::to_string(m) + ": --number-markers " + std::to_string(M) + " exceeds it");
    for (int c = 0; c < 3; ++c)
        for (int k = 0; k < 2; ++k) {
            const std::string path = s.prefix + (k ? ".sl" : ".ss") + SP_CLASS[c];
            const uint64_t size = readable_size(path);
            if (size < 8ull * M)
                fatal("FATAL  : " + path + " holds " + std::to_string(size) + " bytes, fewer than 8 x --number-markers = " + std::to_string(8ull * M));
            std::vector<uint64_t>& v = k ? s.sl[c] : s.ss[c];
            v.resize(M);
            FILE* f = std::fopen(path.c_str(), "rb");
            if (!f || std::fread(v.data(), 8, M, f) != M) fatal("FATAL  : " + path + ": short read");
            std::fclose(f);
        }
    for (int c = 0; c < 3; ++c) {
        const std::string cl = SP_CLASS[c];
        for (unsigned j = 0; j < M; ++j) {
            if (s.sl[c][j] > numInds)
                fatal("FATAL  : " + s.prefix + ".sl" + cl + ": marker " + std::to_string(j) + " lists " + std::to_string(s.sl[c][j]) + " rows, more than N = " +
                      std::to_string(numInds));
            if (s.ss[c][j] > (1ull << 60)) fatal("FATAL  : " + s.prefix + ".ss" + cl + ": marker " + std::to_string(j) + " starts at " + std::to_string(s.ss[c][j]));
            if (j + 1 < M && s.ss[c][j + 1] < s.ss[c][j] + s.sl[c][j])
                fatal("FATAL  : " + s.prefix + ".ss" + cl + ": marker " + std::to_string(j + 1) + " starts at " + std::to_string(s.ss[c][j + 1]) + ", before marker " +
                      std::to_string(j) + " ends (" + std::to_string(s.ss[c][j]) + " + " + std::to_string(s.sl[c][j]) + ")");
        }
        const std::string path = s.prefix + ".si" + cl;
        const uint64_t size = readable_size(path), need = 4 * (s.ss[c][M - 1] + s.sl[c][M - 1]);
        if (size < need)
            fatal("FATAL  : " + path + " holds " + std::to_string(size) + " bytes, fewer than 4 x (ss[last] + sl[last]) = " + std::to_string(need));
    }
    s.on = true;
}

// The sparse files onto the handle (hgibbs_sparse_begin / _put / _end), streamed in slabs of markers of at most 64 MiB a list (a marker
// alone may exceed it): the host never holds more than a slab.  Rows that keep drops or that lie outside [lo, hi) are skipped by the
// library.  Returns the bytes of index lists read.
size_t load_sparse(hgibbs_t dev, size_t numInds, unsigned M, const uint8_t* keep, unsigned lo, unsigned hi, unsigned Ntot)
{
    const SparseSource& s = g_sparse;
    FILE* f[3];
    for (int c = 0; c < 3; ++c)
        if (!(f[c] = std::fopen((s.prefix + ".si" + SP_CLASS[c]).c_str(), "rb"))) fatal("Error: can not open the file [" + s.prefix + ".si" + SP_CLASS[c] + "] to read.");
    hg_check(hgibbs_sparse_begin(dev, (uint32_t)numInds, M, keep, lo, hi, Ntot), "hgibbs_sparse_begin");
    const uint64_t cap = (64ull << 20) / 4;
    std::vector<uint32_t> buf[3];
    size_t bytes = 0;
    for (unsigned j0 = 0; j0 < M;) {
        unsigned j1 = j0 + 1;
        auto fits = [&](unsigned j) {
            for (int c = 0; c < 3; ++c)
                if (s.ss[c][j] + s.sl[c][j] - s.ss[c][j0] > cap) return false;
            return true;
        };
        while (j1 < M && fits(j1)) ++j1;
        hgibbs_sparse_list li[3];
        for (int c = 0; c < 3; ++c) {
            const uint64_t base = s.ss[c][j0], n = s.ss[c][j1 - 1] + s.sl[c][j1 - 1] - base;
            buf[c].resize(n);
            if (fseeko(f[c], (off_t)(4 * base), SEEK_SET) != 0 || std::fread(buf[c].data(), 4, n, f[c]) != n)
                fatal("FATAL  : " + s.prefix + ".si" + SP_CLASS[c] + ": short read");
            li[c] = hgibbs_sparse_list{s.ss[c].data() + j0, s.sl[c].data() + j0, buf[c].data(), base, n};
            bytes += 4 * n;
        }
        hg_check(hgibbs_sparse_put(dev, j0, j1 - j0, &li[0], &li[1], &li[2]), "hgibbs_sparse_put");
        j0 = j1;
    }
    hg_check(hgibbs_sparse_end(dev), "hgibbs_sparse_end");
    for (int c = 0; c < 3; ++c) std::fclose(f[c]);
    return bytes;
}

// The training genotypes as the host holds them before the device takes them: --bfile's .bed, or nothing when they come from the
// sparse files (those are streamed by put_genotypes)
std::vector<uint8_t> read_training(const std::string& prefix, size_t numInds, size_t M)
{
    return g_sparse.on ? std::vector<uint8_t>() : read_bed(prefix, numInds, M);
}

// The genotypes of the kept rows [lo, hi) onto the handle, from either representation (Data::load_data_from_bed_file, data.cpp:671-739,
// resp. load_data_from_sparse_files, :1224-1290): the device image is the same bytes either way.  Returns the bytes read; the host
// copy is released.
size_t put_genotypes(hgibbs_t dev, std::vector<uint8_t>& bed, size_t numInds, unsigned M, const uint8_t* keep, unsigned lo, unsigned hi, unsigned Ntot)
{
    if (g_sparse.on) return load_sparse(dev, numInds, M, keep, lo, hi, Ntot);
    hg_check(hgibbs_load_bed(dev, bed.data(), (numInds + 3) / 4, (uint32_t)numInds, M, keep, lo, hi, Ntot), "hgibbs_load_bed");
    const size_t bytes = bed.size();
    std::vector<uint8_t>().swap(bed);
    return bytes;
}

// Data::readPhenotypeFile(path, numberIndividuals, y), the reader of the route without a .fam (src/main.cpp:96-118): one line per
// individual in file order, numInds lines required; "NA" marks a dropped individual
void read_phen_lines(const std::string& path, size_t numInds, std::vector<double>& y, std::vector<uint8_t>& keep)
{
    std::ifstream in(path);
    if (!in) fatal("Error: can not open the phenotype file [" + path + "] to read.");
    keep.assign(numInds, 1);
    y.clear();
    std::string line;
    size_t lineno = 0;
    while (lineno < numInds && std::getline(in, line)) {
        std::vector<std::string> col = tokens(line, " \t");
        if (col.size() < 3) continue;
        if (col[2] != "NA") y.push_back(std::atof(col[2].c_str()));
        else keep[lineno] = 0;
        ++lineno;
    }
    if (lineno != numInds) fatal("FATAL  : phenotype file covers " + std::to_string(lineno) + " of " + std::to_string(numInds) + " individuals");
}

// the INFO lines of the sparse route
void sparse_info(const Options& opt, int rank, int nranks)
{
    if (rank != 0) return;
    std::printf("INFO   : genotypes are read from the sparse files %s.*\n", g_sparse.prefix.c_str());
    if (!opt.bedFile.empty())
        std::printf("INFO   : --bfile with --sparse-dir/--sparse-basename is hydra's mixed representation, the same numbers twice: this build reads the sparse files and "
                    "takes only .fam/.bim from --bfile\n");
    if (nranks > 1) std::printf("INFO   : each of the %d ranks reads every slab of the sparse files; the library skips the rows outside a rank's shard\n", nranks);
}

// --bed-to-sparse: BayesRRm::write_sparse_data_files, src/BayesRRm.cpp:437-770 -- the whole .bed (every .fam row, NA phenotypes
// included, every .bim marker) as the ten sparse files, compacted on the device (hgibbs_sparse_counts / hgibbs_sparse_get)
int run_bed_to_sparse(const Options& opt, int nranks, int local_rank)
{
    if (nranks > 1) fatal("FATAL  : --bed-to-sparse runs on one process (WORLD_SIZE = " + std::to_string(nranks) + "): one process converts the whole file");
    if (opt.bedFile.empty()) fatal("FATAL  : --bed-to-sparse needs --bfile");
    // directory and name: the pair, else those of --bfile (BayesRRm.cpp:3093-3114)
    const std::string::size_type cut = opt.bedFile.find_last_of('/');
    std::string dir = cut == std::string::npos ? std::string(".") : (cut == 0 ? std::string("/") : opt.bedFile.substr(0, cut));
    std::string bsn = cut == std::string::npos ? opt.bedFile : opt.bedFile.substr(cut + 1);
    if (!opt.sparseDir.empty()) {
        struct stat sb;
        if (stat(opt.sparseDir.c_str(), &sb) != 0 || !S_ISDIR(sb.st_mode))
            fatal("Fatal: requested directory for sparse output (" + opt.sparseDir + ") not found. Must be an existing directory.");
        dir = opt.sparseDir;
        bsn = opt.sparseBsn;
    }
    const std::string prefix = dir + "/" + bsn;
    const size_t N = count_fam(opt.bedFile + ".fam", nullptr), Msz = count_bim(opt.bedFile + ".bim");
    if (N == 0 || Msz == 0 || Msz >= 0x80000000ull) fatal("FATAL  : " + opt.bedFile + ": " + std::to_string(N) + " individuals, " + std::to_string(Msz) + " markers");
    const unsigned M = (unsigned)Msz;
    if (opt.blocksPerRankGiven) std::printf("INFO   : --blocks-per-rank ignored: one process writes the files in slabs of markers\n");
    std::printf("INFO   : will always convert the whole file: N = %zu individuals (NA phenotypes included), M = %u markers\n", N, M);
    std::vector<uint8_t> bed = read_bed(opt.bedFile, N, M);
    const double t0 = now_s();
    hgibbs_t dev = nullptr;
    hg_check(hgibbs_create(local_rank, &dev), "hgibbs_create");
    hg_check(hgibbs_load_bed(dev, bed.data(), (N + 3) / 4, (uint32_t)N, M, nullptr, 0, (uint32_t)N, (uint32_t)std::max<size_t>(N, 2)), "hgibbs_load_bed");
    std::vector<uint8_t>().swap(bed);

    FILE *fl[3], *fs[3], *fi[3];
    for (int c = 0; c < 3; ++c) {
        fl[c] = open_out(prefix + ".sl" + SP_CLASS[c], "wb");
        fs[c] = open_out(prefix + ".ss" + SP_CLASS[c], "wb");
        fi[c] = open_out(prefix + ".si" + SP_CLASS[c], "wb");
    }
    uint64_t at[3] = {0, 0, 0}; // entries written so far: the next marker's absolute start
    const unsigned CH = 65536;  // markers whose counts are fetched together
    const uint64_t cap = (256ull << 20) / 4; // entries of the three lists of a slab together (a marker alone may exceed it)
    std::vector<uint64_t> cnt[3], ss;
    std::vector<uint32_t> idx[3];
    double dev_ms = 0.0;
    for (unsigned m0 = 0; m0 < M; m0 += CH) {
        const unsigned mc = std::min(CH, M - m0);
        for (int c = 0; c < 3; ++c) cnt[c].resize(mc);
        hg_check(hgibbs_sparse_counts(dev, m0, mc, cnt[0].data(), cnt[1].data(), cnt[2].data()), "hgibbs_sparse_counts");
        for (unsigned k0 = 0; k0 < mc;) {
            uint64_t tot[3] = {0, 0, 0};
            unsigned k1 = k0;
            for (; k1 < mc; ++k1) {
                if (k1 > k0 && tot[0] + tot[1] + tot[2] + cnt[0][k1] + cnt[1][k1] + cnt[2][k1] > cap) break;
                for (int c = 0; c < 3; ++c) tot[c] += cnt[c][k1];
            }
            for (int c = 0; c < 3; ++c) idx[c].resize(tot[c]);
            hg_check(hgibbs_sparse_get(dev, m0 + k0, k1 - k0, idx[0].data(), idx[1].data(), idx[2].data()), "hgibbs_sparse_get");
            double ms = 0.0;
            hg_check(hgibbs_last_sparse_ms(dev, nullptr, &ms), "hgibbs_last_sparse_ms");
            dev_ms += ms;
            for (int c = 0; c < 3; ++c) {
                ss.resize(k1 - k0);
                for (unsigned k = k0; k < k1; ++k) {
                    ss[k - k0] = at[c];
                    at[c] += cnt[c][k];
                }
                if (std::fwrite(cnt[c].data() + k0, 8, k1 - k0, fl[c]) != k1 - k0 || std::fwrite(ss.data(), 8, k1 - k0, fs[c]) != k1 - k0 ||
                    std::fwrite(idx[c].data(), 4, tot[c], fi[c]) != tot[c])
                    fatal("FATAL  : short write on " + prefix + ".s??" );
            }
            k0 = k1;
        }
    }
    for (int c = 0; c < 3; ++c) {
        close_out(fl[c], prefix + ".sl" + SP_CLASS[c]);
        close_out(fs[c], prefix + ".ss" + SP_CLASS[c]);
        close_out(fi[c], prefix + ".si" + SP_CLASS[c]);
    }
    FILE* fd = open_out(prefix + ".dim", "w");
    std::fprintf(fd, "%d %d\n", (int)N, (int)M);
    close_out(fd, prefix + ".dim");
    hg_check(hgibbs_destroy(dev), "hgibbs_destroy");
    // the sizes on disk against what was written (check_file_size, BayesRRm.cpp:740-748)
    for (int c = 0; c < 3; ++c) {
        const std::pair<std::string, uint64_t> want[3] = {{".sl", 8ull * M}, {".ss", 8ull * M}, {".si", 4 * at[c]}};
        for (const auto& w : want) {
            const std::string path = prefix + w.first + SP_CLASS[c];
            const uint64_t size = readable_size(path);
            if (size != w.second) fatal("FATAL  : " + path + " holds " + std::to_string(size) + " bytes, " + std::to_string(w.second) + " were written");
        }
    }
    std::printf("INFO   : wrote %s.{dim,sl?,ss?,si?}: %llu + %llu + %llu entries (genotype 1, genotype 2, missing call) in %.3f seconds, %.3f ms of them in the "
                "device's compaction\n",
                prefix.c_str(), (unsigned long long)at[0], (unsigned long long)at[1], (unsigned long long)at[2], now_s() - t0, dev_ms);
    return 0;
}

// ---- restart readers: Data::read_mcmc_output_*_file, src/data.cpp:33-519 ----
struct CsvRestart {
    unsigned iteration_to_restart_from = 0, first_thinned_iteration = 0, first_saved_iteration = 0;
    std::vector<double> sigmaG, pi;
    double sigmaE = 0.0;          // BayesR's
    double mu = 0.0, alpha = 0.0; // BayesW's
};

// data.cpp:406-514: the last line whose iteration is a multiple of --save wins
CsvRestart read_csv_for_restart(const std::string& csv, unsigned thin, unsigned save, int G, int K)
{
    std::ifstream file(csv);
    if (!file) fatal("*FATAL*: failed to open csv file " + csv + "!");
    CsvRestart r;
    r.sigmaG.assign(G, 0.0);
    r.pi.assign((size_t)G * K, 0.0);
    int nSaved = 0, nThinned = 0, last_it = -1;
    std::string str;
    while (std::getline(file, str)) {
        if (str.empty()) continue;
        for (char& ch : str)
            if (ch == ',') ch = ' ';
        char* p = &str[0];
        const long it = std::strtol(p, &p, 10);
        const long ngrp = std::strtol(p, &p, 10);
        last_it = (int)it;
        if (it % thin != 0) fatal("FATAL  : " + csv + ": iteration " + std::to_string(it) + " is not a multiple of --thin");
        if (++nThinned == 1) r.first_thinned_iteration = (unsigned)it;
        if (it % save != 0) continue;
        if (++nSaved == 1) r.first_saved_iteration = (unsigned)it;
        r.iteration_to_restart_from = (unsigned)it;
        if (ngrp != G) fatal("FATAL  : " + csv + ": number of groups differs from this run's");
        for (int g = 0; g < G; ++g) r.sigmaG[g] = std::strtod(p, &p);
        r.sigmaE = std::strtod(p, &p);
        (void)std::strtod(p, &p);      // sigmaG.sum()/(sigmaE+sigmaG.sum())
        (void)std::strtol(p, &p, 10);  // m0
        const long rows = std::strtol(p, &p, 10), cols = std::strtol(p, &p, 10);
        if (rows != G || cols != K) fatal("FATAL  : " + csv + ": pi is " + std::to_string(rows) + "x" + std::to_string(cols) + ", expected " + std::to_string(G) + "x" + std::to_string(K));
        for (size_t i = 0; i < (size_t)G * K; ++i) r.pi[i] = std::strtod(p, &p);
    }
    if (nSaved == 0)
        fatal("FATAL  : No saved iteration could be found when reading " + csv + "!\n       : with last read iteration " + std::to_string(last_it) +
              ", and --thin = " + std::to_string(thin) + " and --save = " + std::to_string(save));
    return r;
}

void pread_at(FILE* f, long off, void* dst, size_t n, const std::string& what)
{
    if (std::fseek(f, off, SEEK_SET) != 0 || std::fread(dst, 1, n, f) != n) fatal("FATAL  : short read from " + what);
}

FILE* open_ro(const std::string& p)
{
    FILE* f = std::fopen(p.c_str(), "rb");
    if (!f) fatal("FATAL  : can not open " + p + " to restart from");
    return f;
}

void expect_u(unsigned got, unsigned want, const std::string& what)
{
    if (got != want) fatal("Mismatch between expected and read " + what + ": " + std::to_string(want) + " vs " + std::to_string(got));
}

// .bet/.cpn history (elem = 8/4 bytes) or the single-line .xbet/.xcpn, data.cpp:256-402
void read_marker_history(const std::string& path, bool xfile, unsigned Mtot, unsigned it_from, unsigned first_thinned, unsigned thin, size_t elem,
                         void* dst)
{
    FILE* f = open_ro(path);
    unsigned Mtot_ = 0, it_ = ~0u;
    pread_at(f, 0, &Mtot_, sizeof(unsigned), path);
    expect_u(Mtot_, Mtot, path + " Mtot");
    if ((it_from - first_thinned) % thin != 0) fatal("FATAL  : " + path + ": restart iteration is not on the --thin grid");
    const long n_skip = (long)((it_from - first_thinned) / thin);
    const long off = xfile ? (long)sizeof(unsigned) : (long)sizeof(unsigned) + n_skip * (long)(sizeof(unsigned) + (size_t)Mtot * elem);
    pread_at(f, off, &it_, sizeof(unsigned), path);
    expect_u(it_, it_from, path + " iteration");
    pread_at(f, off + (long)sizeof(unsigned), dst, (size_t)Mtot * elem, path);
    std::fclose(f);
}

// .eps/.mrk/.gam/.xiv dumps: (iteration, length, payload), data.cpp:33-204
std::vector<uint8_t> read_dump(const std::string& path, unsigned it_from, size_t elem, unsigned* length)
{
    FILE* f = open_ro(path);
    unsigned it_ = ~0u, len = 0;
    pread_at(f, 0, &it_, sizeof(unsigned), path);
    expect_u(it_, it_from, path + " iteration");
    pread_at(f, sizeof(unsigned), &len, sizeof(unsigned), path);
    std::vector<uint8_t> out((size_t)len * elem);
    pread_at(f, 2 * sizeof(unsigned), out.data(), out.size(), path);
    std::fclose(f);
    *length = len;
    return out;
}

// `file >> rng` for boost::mt19937, src/distributions_boost.cpp:46-55: 624 decimal words
void read_rng_file(const std::string& path, hgibbs_rng_state* st)
{
    std::ifstream in(path);
    if (!in) fatal("*FATAL*: Unable to read from file " + path);
    std::vector<uint32_t> w(624);
    for (int i = 0; i < 624; ++i) {
        unsigned long long v = 0;
        if (!(in >> v) || v > 0xffffffffull) fatal("*FATAL*: " + path + " does not hold a boost::mt19937 state");
        w[i] = (uint32_t)v;
    }
    hydra_rng_from_boost_words(w.data(), st);
}

// `file << rng`, src/distributions_boost.cpp:38-44: words separated by single spaces
void write_rng_file(const std::string& path, const hgibbs_rng_state& st)
{
    std::vector<uint32_t> w(624);
    hydra_rng_to_boost_words(&st, w.data());
    std::ofstream out(path, std::ios::out | std::ios::trunc | std::ios::binary);
    if (!out) fatal("FATAL  : can not create " + path);
    for (int i = 0; i < 624; ++i) out << w[i] << (i + 1 < 624 ? " " : "");
}

// Several ranks (one process per GPU, RANK / WORLD_SIZE / LOCAL_RANK in the environment): the RCCL id and the
// IPC handles of the in-launch peer mailboxes travel through files next to the outputs.
void setup_ranks(hgibbs_t dev, const std::string& base, int rank, int nranks)
{
        uint8_t id[128];
        const std::string idf = base + ".ncclid";
        if (rank == 0) {
            hg_check(hgibbs_comm_unique_id(id), "hgibbs_comm_unique_id");
            FILE* f = std::fopen((idf + ".tmp").c_str(), "wb");
            if (!f || std::fwrite(id, 1, 128, f) != 128) fatal("FATAL  : can not write " + idf);
            std::fclose(f);
            std::rename((idf + ".tmp").c_str(), idf.c_str());
        } else {
            FILE* f = nullptr;
            for (int tries = 0; tries < 6000 && !(f = std::fopen(idf.c_str(), "rb")); ++tries)
                std::this_thread::sleep_for(std::chrono::milliseconds(10));
            if (!f || std::fread(id, 1, 128, f) != 128) fatal("FATAL  : can not read " + idf);
            std::fclose(f);
        }
        hg_check(hgibbs_comm_init(dev, nranks, rank, id), "hgibbs_comm_init");
        // in-launch peer-mailbox exchange: every rank publishes its IPC handle next to the id file
        uint8_t mine[64];
        std::vector<uint8_t> all((size_t)nranks * 64);
        bool p2p_ok = hgibbs_p2p_export(dev, mine) == 0;
        {
            const std::string hf = base + ".p2p." + std::to_string(rank);
            FILE* f = std::fopen((hf + ".tmp").c_str(), "wb");
            if (f) {
                std::fwrite(p2p_ok ? "Y" : "N", 1, 1, f);
                std::fwrite(mine, 1, 64, f);
                std::fclose(f);
                std::rename((hf + ".tmp").c_str(), hf.c_str());
            }
        }
        for (int r = 0; r < nranks; ++r) {
            const std::string hf = base + ".p2p." + std::to_string(r);
            FILE* f = nullptr;
            for (int tries = 0; tries < 6000 && !(f = std::fopen(hf.c_str(), "rb")); ++tries)
                std::this_thread::sleep_for(std::chrono::milliseconds(10));
            char flag = 'N';
            if (!f || std::fread(&flag, 1, 1, f) != 1 || std::fread(all.data() + (size_t)r * 64, 1, 64, f) != 64 || flag != 'Y') p2p_ok = false;
            if (f) std::fclose(f);
        }
        if (p2p_ok && hgibbs_p2p_import(dev, all.data()) != 0) p2p_ok = false;
        // a rank that could not import falls back to RCCL; all ranks must agree, so publish the verdict too
        {
            const std::string vf = base + ".p2pok." + std::to_string(rank);
            FILE* f = std::fopen((vf + ".tmp").c_str(), "wb");
            if (f) {
                std::fwrite(p2p_ok ? "Y" : "N", 1, 1, f);
                std::fclose(f);
                std::rename((vf + ".tmp").c_str(), vf.c_str());
            }
            for (int r = 0; r < nranks; ++r) {
                const std::string of = base + ".p2pok." + std::to_string(r);
                FILE* g = nullptr;
                for (int tries = 0; tries < 6000 && !(g = std::fopen(of.c_str(), "rb")); ++tries)
                    std::this_thread::sleep_for(std::chrono::milliseconds(10));
                char flag = 'N';
                if (!g || std::fread(&flag, 1, 1, g) != 1 || flag != 'Y') p2p_ok = false;
                if (g) std::fclose(g);
            }
        }
        hg_check(hgibbs_set_option(dev, "p2p", p2p_ok ? 1 : 0), "p2p");
        if (rank == 0) std::printf("INFO   : per-batch exchange over %s\n", p2p_ok ? "xGMI peer mailboxes (in-launch)" : "RCCL all-reduce");
        if (rank == 0) {
            std::this_thread::sleep_for(std::chrono::milliseconds(500));
            std::remove(idf.c_str());
            for (int r = 0; r < nranks; ++r) {
                std::remove((base + ".p2p." + std::to_string(r)).c_str());
                std::remove((base + ".p2pok." + std::to_string(r)).c_str());
            }
        }
}

// ---- what the samplers' command lines share (main for bayesMPI, run_bayesw, and run_sumstats from its chain down) ----
// Each sampler keeps its own loop; these are the pieces of it that are the same, written once.

// N and M before the phenotypes are read: the .fam/.bim of --bfile, or, on the sparse route (main.cpp:96-118), the options'
struct Dims {
    size_t numInds = 0, numSnps = 0;
    std::vector<std::string> fam_ids;
};

Dims read_dims(const Options& opt)
{
    const bool haveBed = !opt.bedFile.empty();
    if (!haveBed && opt.numberIndividuals == 0) fatal("FATAL  : opt.numberIndividuals is zero! Set it via --number-individuals in call.");
    if (!haveBed && opt.numberMarkers == 0) fatal("FATAL  : opt.numberMarkers is zero! Set it via --number-markers in call.");
    Dims d;
    d.numInds = haveBed ? count_fam(opt.bedFile + ".fam", &d.fam_ids) : opt.numberIndividuals;
    d.numSnps = haveBed ? count_bim(opt.bedFile + ".bim") : opt.numberMarkers;
    return d;
}

// ... and the options against them, once the phenotypes are read; returns Mtot
unsigned check_dims(const Options& opt, const Dims& d)
{
    if (opt.numberIndividuals == 0) fatal("FATAL  : opt.numberIndividuals is zero! Set it via --number-individuals in call.");
    if (opt.numberMarkers == 0) fatal("FATAL  : opt.numberMarkers is zero! Set it via --number-markers in call.");
    if (opt.numberIndividuals != d.numInds) fatal("FATAL  : --number-individuals does not match the .fam file");
    const unsigned Mtot = opt.numberMarkers;
    if (Mtot > d.numSnps) fatal("FATAL  : --number-markers exceeds the .bim file");
    return Mtot;
}

// The groups and their mixtures from --groupIndexFile/--groupMixtureFile, or the one row of --S behind a zero
struct Mixtures {
    std::vector<int32_t> groups; // empty: one group
    std::vector<double> mS_flat; // G x K
    int G = 0, K = 0;
};

Mixtures read_mixtures(const Options& opt, unsigned Mtot, bool positiveS)
{
    Mixtures m;
    std::vector<std::vector<double>> mS;
    if (!opt.groupIndexFile.empty()) { // src/BayesW.cpp:773-776
        m.groups = read_groups(opt.groupIndexFile);
        mS = read_mS(opt.groupMixtureFile);
        if (m.groups.size() < Mtot) fatal("FATAL  : group file covers fewer markers than --number-markers");
        m.groups.resize(Mtot);
    } else {
        std::vector<double> row{0.0};
        for (double v : opt.S) {
            if (positiveS && v <= 0.0) fatal("FATAL  : mixture value can only be strictly positive");
            row.push_back(v);
        }
        mS.push_back(row);
    }
    m.G = (int)mS.size();
    m.K = (int)mS[0].size();
    for (auto& r : mS) m.mS_flat.insert(m.mS_flat.end(), r.begin(), r.end());
    return m;
}

// --save becomes a multiple of --thin (BayesRRm.cpp:1058-1066, BayesW.cpp:981-989).  BayesW says so on every rank and in one
// line more than BayesR.
void adjust_save(Options& opt, bool say, bool sayNotMultiple)
{
    if (opt.save < opt.thin) {
        opt.save = opt.thin;
        if (say) std::printf("WARNING: opt.save was lower that opt.thin ; opt.save reset to opt.thin (%d)\n", opt.thin);
    }
    if (opt.save % opt.thin != 0) {
        if (say && sayNotMultiple) std::printf("WARNING: opt.save (= %d) was not a multiple of opt.thin (= %d)\n", opt.save, opt.thin);
        opt.save = (opt.save / opt.thin) * opt.thin;
        if (say) std::printf("         opt.save reset to %d, the closest multiple of opt.thin (%d)\n", opt.save, opt.thin);
    }
}

// This rank's rows [lo, hi) of the Ntot kept ones: individuals are sharded in multiples of 4
struct Shard {
    unsigned lo = 0, hi = 0;
    unsigned rows() const { return hi - lo; }
};

Shard shard_of(unsigned Ntot, int rank, int nranks)
{
    const unsigned per = ((Ntot + nranks - 1) / nranks + 3) / 4 * 4;
    return {std::min(Ntot, rank * per), std::min(Ntot, (rank + 1) * per)};
}

// A sampler's handle: among its ranks, with this build's tuning knobs (cpg 0: BayesW has no column groups to size)
hgibbs_t open_device(const Options& opt, const std::string& base, int rank, int nranks, int local_rank, int cpg)
{
    hgibbs_t dev = nullptr;
    hg_check(hgibbs_create(local_rank, &dev), "hgibbs_create");
    if (nranks > 1) setup_ranks(dev, base, rank, nranks);
    if (opt.batch) hg_check(hgibbs_set_option(dev, "batch", opt.batch), "batch");
    if (cpg) hg_check(hgibbs_set_option(dev, "cols_per_group", cpg), "cols_per_group");
    return dev;
}

// Data::load_data_from_bed_file, data.cpp:671-739: this rank's shard of the training genotypes, and what it took
void load_and_report(hgibbs_t dev, const Options& opt, size_t numInds, unsigned Mtot, const uint8_t* keep, const Shard& sh, unsigned Ntot, int rank)
{
    const double tl0 = now_s();
    std::vector<uint8_t> bed = read_training(opt.bedFile, numInds, Mtot);
    const size_t bytes = put_genotypes(dev, bed, numInds, Mtot, keep, sh.lo, sh.hi, Ntot);
    std::printf("INFO   : rank %3d took %.3f seconds to load  %lu bytes  =>  BW = %7.3f GB/s\n", rank, now_s() - tl0, (unsigned long)bytes,
                (double)bytes * 1e-9 / (now_s() - tl0));
}

// The output files of one run, opened truncated and closed together
struct OutFiles {
    std::vector<std::pair<FILE*, std::string>> files;
    FILE* open(const std::string& p)
    {
        files.emplace_back(open_out(p, "wb+"), p);
        return files.back().first;
    }
    void close(bool checked) // checked: a failing close is a short write on that file
    {
        for (auto& f : files)
            if (checked) close_out(f.first, f.second);
            else std::fclose(f.first);
    }
};

// .bet/.acu/.cpn: the marker count at 0 (the caller's), then per thinned iteration (iteration, M elements)
void write_thinned(FILE* f, unsigned n_thinned_saved, unsigned iteration, const void* v, unsigned M, size_t elem)
{
    const long off = sizeof(unsigned) + (long)n_thinned_saved * (sizeof(unsigned) + (long)M * elem);
    pwrite_at(f, off, &iteration, sizeof(unsigned));
    pwrite_at(f, off + sizeof(unsigned), v, (size_t)M * elem);
}

// .mus.<rank>: (iteration, mu) per thinned iteration
void write_mus(FILE* f, unsigned n_thinned_saved, unsigned iteration, double mu)
{
    const long off = (long)n_thinned_saved * (sizeof(unsigned) + sizeof(double));
    pwrite_at(f, off, &iteration, sizeof(unsigned));
    pwrite_at(f, off + sizeof(unsigned), &mu, sizeof(double));
}

// .csv/.gam text: line n of lines of one length
void write_line(FILE* f, unsigned n_thinned_saved, const char* line, int len)
{
    pwrite_at(f, (long)n_thinned_saved * len, line, (size_t)len);
}

// .eps/.mrk/.gam.<rank>/.xiv dumps, overwritten at every save: (iteration, length, payload)
void write_dump(FILE* f, unsigned iteration, unsigned length, const void* v, size_t elem)
{
    pwrite_at(f, 0, &iteration, sizeof(unsigned));
    pwrite_at(f, sizeof(unsigned), &length, sizeof(unsigned));
    pwrite_at(f, 2 * sizeof(unsigned), v, (size_t)length * elem);
}

// .xbet/.xcpn, overwritten at every save: the marker count at 0 (the caller's), the iteration, M elements
void write_xfile(FILE* f, unsigned iteration, const void* v, unsigned M, size_t elem)
{
    pwrite_at(f, sizeof(unsigned), &iteration, sizeof(unsigned));
    pwrite_at(f, 2 * sizeof(unsigned), v, (size_t)M * elem);
}

// What a restart reads the same way for BayesR and BayesW.  Two readers and not one: BayesR reads its .mus between them, and the
// order of the reads is the order in which bad files are refused.
struct RestartState {
    std::vector<double> beta;
    std::vector<int32_t> comp;
    std::vector<uint8_t> eps_dump, order_dump;
    const double* eps = nullptr; // this rank's rows in eps_dump: a full-length dump (hydra's own, or a 1-rank run's) is sliced
    const int32_t* order() const { return (const int32_t*)order_dump.data(); }
};

// beta and the components of iteration it_from, from the histories or, with the x-file switch, from .xbet/.xcpn
void read_restart_effects(RestartState& r, const Options& opt, const std::string& base_in, unsigned Mtot, unsigned it_from, unsigned first_thinned)
{
    const bool xf = opt.useXfilesInRestart;
    r.beta.resize(Mtot);
    r.comp.resize(Mtot);
    read_marker_history(base_in + (xf ? ".xbet" : ".bet"), xf, Mtot, it_from, first_thinned, opt.thin, sizeof(double), r.beta.data());
    read_marker_history(base_in + (xf ? ".xcpn" : ".cpn"), xf, Mtot, it_from, first_thinned, opt.thin, sizeof(int32_t), r.comp.data());
}

// .eps.<rank> and .mrk.<rank>
void read_restart_shard(RestartState& r, const std::string& base_in, int rank, unsigned it_from, unsigned Ntot, const Shard& sh, unsigned Mtot)
{
    unsigned len = 0;
    r.eps_dump = read_dump(base_in + ".eps." + std::to_string(rank), it_from, sizeof(double), &len);
    r.eps = (const double*)r.eps_dump.data();
    if (len == Ntot && len != sh.rows()) r.eps += sh.lo;
    else expect_u(len, sh.rows(), ".eps Ntot");
    r.order_dump = read_dump(base_in + ".mrk." + std::to_string(rank), it_from, sizeof(int32_t), &len);
    expect_u(len, Mtot, ".mrk M");
}

void print_restart_banner(const std::string& base_in, unsigned it_from, unsigned iteration_start) // Data::print_restart_banner, data.cpp:20-31
{
    const std::string stars(100, '*');
    std::printf("INFO   : %s\nINFO   : RESTART DETECTED\nINFO   : restarting from: %s.* files\n", stars.c_str(), base_in.c_str());
    std::printf("INFO   : last saved iteration:        %d\nINFO   : will restart from iteration: %d\nINFO   : %s\n", it_from, iteration_start, stars.c_str());
}

// BayesW's .csv (src/data.cpp:523-622): the last line whose iteration is a multiple of --save wins
CsvRestart read_csv_for_restart_w(const std::string& csv, unsigned thin, unsigned save, int G, int K)
{
    std::ifstream file(csv);
    if (!file) fatal("*FATAL*: failed to open csv file " + csv + "!");
    CsvRestart r;
    r.sigmaG.assign(G, 0.0);
    r.pi.assign((size_t)G * K, 0.0);
    int nSaved = 0, nThinned = 0;
    std::string str;
    while (std::getline(file, str)) {
        if (str.empty()) continue;
        for (char& ch : str)
            if (ch == ',') ch = ' ';
        char* q = &str[0];
        const long it = std::strtol(q, &q, 10);
        if (it % thin != 0) fatal("FATAL  : " + csv + ": iteration " + std::to_string(it) + " is not a multiple of --thin");
        if (++nThinned == 1) r.first_thinned_iteration = (unsigned)it;
        if (it % save != 0) continue;
        ++nSaved;
        r.iteration_to_restart_from = (unsigned)it;
        r.mu = std::strtod(q, &q);
        (void)std::strtod(q, &q); // sigmaG.sum()
        r.alpha = std::strtod(q, &q);
        (void)std::strtod(q, &q); // h2
        (void)std::strtol(q, &q, 10); // m0
        const long rows = std::strtol(q, &q, 10), cols = std::strtol(q, &q, 10);
        if (rows != G || cols != K) fatal("FATAL  : " + csv + ": pi is " + std::to_string(rows) + "x" + std::to_string(cols) + ", expected " + std::to_string(G) + "x" + std::to_string(K));
        for (int g = 0; g < G; ++g) r.sigmaG[g] = std::strtod(q, &q);
        for (size_t i = 0; i < (size_t)G * K; ++i) r.pi[i] = std::strtod(q, &q);
    }
    if (nSaved == 0) fatal("FATAL  : No saved iteration could be found when reading " + csv + "!");
    return r;
}

// BayesW's text .gam: the last line whose iteration is a multiple of --save (src/data.cpp:624-663), which must be it_from
std::vector<double> read_gam_for_restart_w(const std::string& gam, unsigned save, int C, unsigned it_from)
{
    std::ifstream gf(gam);
    if (!gf) fatal("*FATAL*: failed to open csv file " + gam + "!");
    std::vector<double> gamma(C);
    long g_it = -1;
    std::string str;
    while (std::getline(gf, str)) {
        if (str.empty()) continue;
        for (char& ch : str)
            if (ch == ',') ch = ' ';
        char* q = &str[0];
        const long it = std::strtol(q, &q, 10);
        if (it % save != 0) continue;
        g_it = it;
        for (int i = 0; i < C; ++i) gamma[i] = std::strtod(q, &q);
    }
    expect_u((unsigned)g_it, it_from, ".gam iteration");
    return gamma;
}

// Data::readPhenFailFiles / readPhenFailCovFiles, src/data.cpp:1681-1802: .phen, .fail (and .cov)
// are read line by line in lockstep; an individual is dropped if its phenotype is NA, its failure
// indicator is -9, or any covariate is NA.
void read_phen_fail(const std::string& phen, const std::string& failf, const std::string& cov, size_t numInds, std::vector<double>& y,
                    std::vector<int32_t>& fail, std::vector<uint8_t>& keep, std::vector<double>& X, int& C)
{
    std::ifstream inp(phen), inf(failf), inc;
    if (!inp) fatal("Error: can not open the phenotype file [" + phen + "] to read.");
    if (!inf) fatal("Error: can not open the failure file [" + failf + "] to read.");
    if (!cov.empty()) {
        inc.open(cov);
        if (!inc) fatal("Error: can not open the covariates file [" + cov + "] to read.");
    }
    keep.assign(numInds, 1);
    y.clear();
    fail.clear();
    X.clear();
    std::string lp, lf, lc;
    size_t line = 0;
    while (std::getline(inp, lp)) {
        if (!std::getline(inf, lf)) fatal("FATAL  : failure file is shorter than the phenotype file");
        if (!cov.empty() && !std::getline(inc, lc)) fatal("FATAL  : covariates file is shorter than the phenotype file");
        if (line >= numInds) break;
        std::vector<std::string> cp = tokens(lp, " \t"), cf = tokens(lf, " \t"), cc = tokens(lc, " \t");
        if (cp.size() < 3 || cf.empty()) continue;
        bool naC = false;
        for (size_t i = 2; i < cc.size(); ++i)
            if (cc[i] == "NA") naC = true;
        if (cp[2] != "NA" && !naC && cf[0] != "-9") {
            y.push_back(std::atof(cp[2].c_str()));
            const double d = std::atof(cf[0].c_str());
            if (d != 0.0 && d != 1.0) fatal("FATAL  : failure indicator on line " + std::to_string(line) + " is neither 0, 1 nor -9");
            fail.push_back((int32_t)d);
            for (size_t i = 2; i < cc.size(); ++i) X.push_back(std::stod(cc[i]));
        } else {
            std::cout << "NA(s) detected on line " << line << ", naP? " << cp[2] << ", naF? " << cf[0] << std::endl;
            keep[line] = 0;
        }
        ++line;
    }
    if (line != numInds) fatal("FATAL  : phenotype/failure files cover " + std::to_string(line) + " of " + std::to_string(numInds) + " individuals");
    C = (y.empty() || cov.empty()) ? 0 : (int)(X.size() / y.size());
}

// --mpibayes bayesWMPI: BayesW::runMpiGibbs_bW, src/BayesW.cpp:905-2176
int run_bayesw(const Options& opt_in, int rank, int nranks, int local_rank)
{
    Options opt = opt_in;
    if (opt.failureFile.empty()) fatal("FATAL  : --failure is mandatory with --mpibayes bayesWMPI");
    if (opt.quad_points.empty()) fatal("Possible number of quad_points = 3,5,7,9,11,13,15,17,25"); // src/BayesW.cpp:706-708
    const int quad = std::atoi(opt.quad_points.c_str());
    const Dims dims = read_dims(opt); // without --bfile the files are read line by line
    const size_t numInds = dims.numInds;
    std::vector<double> y, covX;
    std::vector<int32_t> fail;
    std::vector<uint8_t> keep;
    int C = 0;
    read_phen_fail(opt.phenotypeFile, opt.failureFile, opt.covariates ? opt.covariatesFile : std::string(), numInds, y, fail, keep, covX, C);
    const unsigned numNAs = (unsigned)(numInds - y.size());
    const unsigned Mtot = check_dims(opt, dims);
    const unsigned Ntot = (unsigned)numInds - numNAs;
    std::printf("INFO   : Full dataset includes Mtot=%d markers and Ntot=%d individuals.\n", Mtot, (int)numInds);
    if (use_sparse(opt)) {
        open_sparse(opt, numInds, Mtot);
        sparse_info(opt, rank, nranks);
    }

    const Mixtures mix = read_mixtures(opt, Mtot, false);
    const int G = mix.G, K = mix.K;
    std::printf("numGroups = %d, data.groups.size() = %lu, Mtot = %d\n", G, (unsigned long)Mtot, Mtot); // :778
    adjust_save(opt, true, true);
    make_out_dir(opt);
    const std::string base_in = opt.mcmcOutDir + "/" + opt.mcmcOutNam; // a restart reads <name>.*, writes <name>_rs.* (:994-1008)
    const std::string base = opt.restart ? base_in + "_rs" : base_in;

    hgibbs_t dev = open_device(opt, base, rank, nranks, local_rank, 0);
    const Shard sh = shard_of(Ntot, rank, nranks);
    load_and_report(dev, opt, numInds, Mtot, numNAs ? keep.data() : nullptr, sh, Ntot, rank);
    if (numNAs) std::printf("INFO   : Ntot adjusted by -%d to account for NAs in phenotype file. Now Ntot=%d\n", numNAs, Ntot);

    hydraw_model_desc md{};
    md.seed = opt.seed;
    md.shuffle = opt.shuffleMarkers;
    md.G = G;
    md.K = K;
    md.groups = mix.groups.empty() ? nullptr : mix.groups.data();
    md.mS = mix.mS_flat.data();
    md.quad_points = quad;
    hydraw_chain_t chain = nullptr;
    hg_check(hydraw_chain_create(dev, &md, y.data(), fail.data(), &chain), "hydraw_chain_create");
    if (opt.covariates) hg_check(hydraw_chain_set_covariates(chain, covX.data(), C), "hydraw_chain_set_covariates");

    // ---- --restart: BayesW::init_from_restart, src/BayesW.cpp:869-903 (readers src/data.cpp:523-663) ----
    unsigned iteration_start = 0;
    if (opt.restart) {
        std::printf("RESTART: from files: %s.* files\n", base_in.c_str());
        const CsvRestart cr = read_csv_for_restart_w(base_in + ".csv", opt.thin, opt.save, G, K);
        const unsigned it_from = cr.iteration_to_restart_from;
        if (it_from == 0) fatal("FATAL  : There is no point in restarting a chain from iteration 0 (not saved anyway)\n         => restart your analysis from scratch");
        RestartState r;
        read_restart_effects(r, opt, base_in, Mtot, it_from, cr.first_thinned_iteration);
        read_restart_shard(r, base_in, rank, it_from, Ntot, sh, Mtot);
        std::vector<double> r_gamma;
        std::vector<uint8_t> xb;
        if (opt.covariates) {
            r_gamma = read_gam_for_restart_w(base_in + ".gam", opt.save, C, it_from);
            unsigned len = 0;
            xb = read_dump(base_in + ".xiv", it_from, sizeof(int32_t), &len);
            expect_u(len, (unsigned)C, ".xiv length");
        }
        hydraw_restart_state rs{};
        rs.iteration = it_from;
        rs.mu = cr.mu;
        rs.alpha = cr.alpha;
        rs.sigmaG = cr.sigmaG.data();
        rs.pi = cr.pi.data();
        rs.beta = r.beta.data();
        rs.components = r.comp.data();
        rs.eps = r.eps;
        rs.order = r.order();
        rs.gamma = opt.covariates ? r_gamma.data() : nullptr;
        rs.xI = opt.covariates ? (const int32_t*)xb.data() : nullptr;
        rs.ars_seed = opt.seed + it_from; // srand(opt.seed + iteration_to_restart_from), :877
        read_rng_file(base_in + ".rng." + std::to_string(rank), &rs.rng);
        hg_check(hydraw_chain_restore(chain, &rs), "hydraw_chain_restore");
        iteration_start = it_from + 1;
        print_restart_banner(base_in, it_from, iteration_start);
    }

    OutFiles outs;
    // the shared files are rank 0's (every rank holds the same chain); the others write theirs into the void
    auto open_shared = [&](const std::string& p) { return outs.open(rank == 0 ? p : std::string("/dev/null")); };
    FILE* outf = open_shared(base + ".csv");
    FILE* betf = open_shared(base + ".bet");
    FILE* cpnf = open_shared(base + ".cpn");
    FILE* xbetf = open_shared(base + ".xbet");
    FILE* xcpnf = open_shared(base + ".xcpn");
    FILE* gamf = open_shared(base + ".gam"); // text, one line per thinned iteration (:1966-1977)
    FILE* xivf = open_shared(base + ".xiv");
    FILE* epsf = outs.open(base + ".eps." + std::to_string(rank));
    FILE* mrkf = outs.open(base + ".mrk." + std::to_string(rank));
    for (FILE* f : {betf, xbetf, cpnf, xcpnf}) pwrite_at(f, 0, &Mtot, sizeof(unsigned)); // :1096-1101

    std::vector<double> beta(Mtot), eps(sh.rows()), sigmaG(G), gamma(C);
    std::vector<int32_t> comp(Mtot), m0(G), xiv(C);
    std::vector<char> buff(50000);
    unsigned n_thinned_saved = 0;
    const double t_all = now_s();
    for (unsigned iteration = iteration_start; iteration < opt.chainLength; ++iteration) {
        const double t0 = now_s();
        hg_check(hydraw_chain_iterate(chain), "hydraw_chain_iterate");
        const double t1 = now_s();
        double mu = 0, alpha = 0;
        hydraw_chain_state(chain, &mu, &alpha, sigmaG.data(), nullptr, m0.data(), nullptr, nullptr, nullptr);
        double sg = 0;
        long m0s = 0;
        for (int g = 0; g < G; ++g) {
            sg += sigmaG[g];
            m0s += m0[g];
        }
        if (rank == 0) std::printf("%u. %ld; %.7g; %.7g; %.7g\n", iteration, m0s, mu, alpha, sg); // :1906-1908
        if (rank == 0) std::printf("RESULT : it %4d, rank %4d: proc = %9.3f s, sync = %9.3f (%9.3f + %9.3f), n_sync = %8d (%8d + %8d) (%7.3f / %7.3f), "
                    "betasq = %15.10f, m0 = %10d\n",
                    iteration, rank, t1 - t0, 0.0, 0.0, 0.0, 0, 0, 0, 0.0, 0.0, 0.0, (int)m0s);
        std::fflush(stdout);

        if (iteration % opt.thin == 0) { // :1937-2019
            const int len = hydraw_chain_csv_line(chain, iteration, buff.data(), buff.size());
            write_line(outf, n_thinned_saved, buff.data(), len);
            if (opt.covariates) {
                hydraw_chain_gamma(chain, gamma.data(), xiv.data());
                std::string gl(64 + 32 * (size_t)C, '\0');
                int n = std::snprintf(&gl[0], gl.size(), "%5d", iteration);
                for (int ii = 0; ii < C; ++ii) n += std::snprintf(&gl[n], gl.size() - n, ", %20.17f", gamma[ii]);
                n += std::snprintf(&gl[n], gl.size() - n, "\n");
                write_line(gamf, n_thinned_saved, gl.data(), n);
                if (iteration > 0 && iteration % opt.save == 0) write_dump(xivf, iteration, (unsigned)C, xiv.data(), sizeof(int));
            }
            hg_check(hgibbs_w_get_beta(dev, beta.data(), comp.data()), "hgibbs_w_get_beta");
            write_thinned(betf, n_thinned_saved, iteration, beta.data(), Mtot, sizeof(double));
            write_thinned(cpnf, n_thinned_saved, iteration, comp.data(), Mtot, sizeof(int));
            n_thinned_saved += 1;
        }
        if (iteration > 0 && iteration % opt.save == 0) { // :2028-2052
            hg_check(hydraw_chain_reseed_ars(chain, opt.seed + iteration), "hydraw_chain_reseed_ars"); // srand(opt.seed + iteration)
            hgibbs_rng_state rst;
            hydraw_chain_state(chain, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &rst, nullptr);
            write_rng_file(base + ".rng." + std::to_string(rank), rst);
            hg_check(hgibbs_get_residual(dev, eps.data()), "hgibbs_get_residual");
            hg_check(hgibbs_w_get_beta(dev, beta.data(), comp.data()), "hgibbs_w_get_beta");
            write_dump(epsf, iteration, sh.rows(), eps.data(), sizeof(double)); // this rank's rows
            write_dump(mrkf, iteration, Mtot, hydraw_chain_order(chain), sizeof(int));
            write_xfile(xbetf, iteration, beta.data(), Mtot, sizeof(double));
            write_xfile(xcpnf, iteration, comp.data(), Mtot, sizeof(int));
        }
    }
    std::printf("INFO   : rank %4d, time to process the data: %.3f sec\n", rank, now_s() - t_all);
    outs.close(false);
    hydraw_chain_destroy(chain);
    hgibbs_destroy(dev);
    return 0;
}

// ---- --predict-bfile: score a target cohort with the chain's effects ----
struct BimRows {
    std::vector<std::string> id, a1, a2;
    std::vector<std::string> chr; // (--ld-window)
    std::vector<long long> bp;
};

BimRows read_bim(const std::string& path, size_t limit)
{
    std::ifstream in(path);
    if (!in) fatal("Error: can not open the file [" + path + "] to read.");
    BimRows b;
    std::string chr, id, gpos, pos, a1, a2;
    while (b.id.size() < limit && in >> chr >> id >> gpos >> pos >> a1 >> a2) {
        b.id.push_back(id);
        b.a1.push_back(a1);
        b.a2.push_back(a2);
        b.chr.push_back(chr);
        b.bp.push_back(std::atoll(pos.c_str()));
    }
    return b;
}

// <dir>/<name>.bet: u32 Mtot, then (u32 iteration, Mtot f64) per thinned iteration (postproc/beta_converter.cpp); the records whose
// iteration is at least `burnin`
void read_bet_records(const std::string& path, unsigned Mtot, unsigned burnin, std::vector<unsigned>& its, std::vector<double>& beta,
                      const char* why = "--predict-bfile scores with the chain's effects")
{
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) fatal("FATAL  : can not open " + path + " (" + why + ": run the chain first)");
    unsigned m = 0;
    if (std::fread(&m, sizeof m, 1, f) != 1 || m != Mtot) {
        std::fclose(f);
        fatal("FATAL  : " + path + " holds " + std::to_string(m) + " markers, --number-markers says " + std::to_string(Mtot));
    }
    std::vector<double> row(Mtot);
    unsigned it = 0, total = 0;
    while (std::fread(&it, sizeof it, 1, f) == 1) {
        if (std::fread(row.data(), sizeof(double), Mtot, f) != Mtot) break; // (a record cut short: the chain was stopped while writing)
        ++total;
        if (it < burnin) continue;
        its.push_back(it);
        beta.insert(beta.end(), row.begin(), row.end());
    }
    std::fclose(f);
    if (its.empty())
        fatal("FATAL  : " + path + ": no record at or after --burn-in " + std::to_string(burnin) + " (" + std::to_string(total) + " records)");
}

// Named sets of markers (--pve, --ld-score, --assoc-sets)
struct MarkerSets {
    std::vector<std::string> name;
    std::vector<std::vector<uint32_t>> idx; // markers of each set, increasing
};

// The SETNAME SNPID file of --pve-sets, --ld-score-sets and --assoc-sets: the sets in the order in which the file first names them.
// unknown: null refuses an id the .bim lacks; otherwise such an id is counted there and left out (a set may end up empty).
MarkerSets read_sets_file(const std::string& path, const std::string& bedFile, const BimRows& bim, unsigned Mtot, size_t* unknown = nullptr)
{
    MarkerSets ms;
    std::ifstream in(path);
    if (!in) fatal("Error: can not open the file [" + path + "] to read.");
    std::map<std::string, uint32_t> snp;
    for (unsigned j = 0; j < Mtot; ++j) snp.emplace(bim.id[j], j);
    std::map<std::string, size_t> at;
    std::map<std::pair<size_t, uint32_t>, int> seen;
    std::string line;
    size_t lineno = 0;
    while (std::getline(in, line)) {
        ++lineno;
        const std::vector<std::string> col = tokens(line, " \t\r");
        if (col.empty()) continue;
        const std::string where = "FATAL  : " + path + " line " + std::to_string(lineno) + ": ";
        if (col.size() != 2) fatal(where + "expected SETNAME SNPID");
        const auto j = snp.find(col[1]);
        if (j == snp.end() && !unknown) fatal(where + "SNP " + col[1] + " is not among the first " + std::to_string(Mtot) + " markers of " + bedFile + ".bim");
        auto it = at.find(col[0]);
        if (it == at.end()) {
            ms.name.push_back(col[0]);
            ms.idx.emplace_back();
            it = at.emplace(col[0], ms.idx.size() - 1).first;
        }
        if (j == snp.end()) {
            ++*unknown;
            continue;
        }
        if (!seen.emplace(std::make_pair(it->second, j->second), 1).second) fatal(where + "SNP " + col[1] + " is given twice for set " + col[0]);
        ms.idx[it->second].push_back(j->second);
    }
    if (ms.idx.empty()) fatal("FATAL  : " + path + " names no set");
    for (auto& r : ms.idx) std::sort(r.begin(), r.end());
    return ms;
}

// The groups of --pve-groups and --ld-score-groups: one set per group number of the group index file, in ascending order of the number
MarkerSets sets_from_groups(const Options& opt, unsigned Mtot)
{
    MarkerSets ms;
    const std::vector<int32_t> groups = read_groups(opt.groupIndexFile);
    if (groups.size() < Mtot) fatal("FATAL  : group file covers fewer markers than --number-markers");
    std::map<int32_t, size_t> at;
    for (unsigned j = 0; j < Mtot; ++j) at.emplace(groups[j], 0);
    for (auto& g : at) {
        g.second = ms.idx.size();
        ms.name.push_back("group" + std::to_string(g.first));
        ms.idx.emplace_back();
    }
    for (unsigned j = 0; j < Mtot; ++j) ms.idx[at[groups[j]]].push_back(j);
    return ms;
}

// The chain's cohort as every analysis mode takes it: the rows that kept their phenotype (and, with --covariates, every covariate)
// of the first Mtot markers of --bfile
struct Cohort {
    const std::vector<uint8_t>& keep; // per .fam row
    unsigned numInds, numNAs, Ntot;   // .fam rows, dropped rows, the chain's rows
    unsigned Mtot;
    int local_rank;
};

// A handle on the chain's rows, as one shard, from the training genotypes (read_training: --bfile's .bed, or the sparse files); the
// host copy is released
hgibbs_t open_training(const Cohort& co, std::vector<uint8_t>& bed)
{
    hgibbs_t dev = nullptr;
    hg_check(hgibbs_create(co.local_rank, &dev), "hgibbs_create");
    (void)put_genotypes(dev, bed, co.numInds, co.Mtot, co.numNAs ? co.keep.data() : nullptr, 0, co.Ntot, co.Ntot);
    return dev;
}

int run_predict(const Options& opt, const Cohort& co)
{
    const std::string base = opt.mcmcOutDir + "/" + opt.mcmcOutNam;
    const std::string out = opt.predictOut.empty() ? base + ".prs" : opt.predictOut;
    const BimRows tr = read_bim(opt.bedFile + ".bim", co.Mtot);
    std::vector<unsigned> its;
    std::vector<double> betas;
    read_bet_records(base + ".bet", co.Mtot, opt.burnin, its, betas);
    const size_t S = its.size();

    // target cohort: .fam (every row: the target needs no phenotype), .bim matched to the training markers by id
    const std::string tp = opt.predictBfile;
    const FamIds tfam = read_fam_ids(tp + ".fam", (size_t)-1, nullptr);
    const size_t nT = tfam.fid.size();
    if (nT == 0) fatal("FATAL  : " + tp + ".fam lists no individual");
    const BimRows tg = read_bim(tp + ".bim", (size_t)-1);
    const size_t Mt = tg.id.size();
    std::map<std::string, unsigned> train_idx;
    for (unsigned j = 0; j < co.Mtot; ++j)
        if (!train_idx.emplace(tr.id[j], j).second) fatal("FATAL  : the training .bim lists SNP id " + tr.id[j] + " twice: markers are matched by id");
    std::map<std::string, int> seen;
    std::vector<int> match(Mt, -1); // training marker of each target column, -1 = contributes nothing
    std::vector<uint8_t> flip(Mt, 0);
    size_t same = 0, swapped = 0, allele = 0, absent = 0;
    for (size_t t = 0; t < Mt; ++t) {
        if (!seen.emplace(tg.id[t], 1).second) fatal("FATAL  : " + tp + ".bim lists SNP id " + tg.id[t] + " twice: markers are matched by id");
        const auto it = train_idx.find(tg.id[t]);
        if (it == train_idx.end()) {
            ++absent;
            continue;
        }
        const unsigned j = it->second;
        if (tg.a1[t] == tr.a1[j] && tg.a2[t] == tr.a2[j]) {
            match[t] = (int)j;
            ++same;
        } else if (tg.a1[t] == tr.a2[j] && tg.a2[t] == tr.a1[j]) {
            match[t] = (int)j;
            flip[t] = 1;
            ++swapped;
        } else
            ++allele;
    }
    std::printf("PREDICT: %zu target markers: %zu matched (%zu same alleles, %zu swapped), %zu allele mismatch, %zu not in training; "
                "%zu of %u training markers unused\n",
                Mt, same + swapped, same, swapped, allele, absent, (size_t)co.Mtot - same - swapped, co.Mtot);
    std::printf("PREDICT: %zu records of %s (iterations %u .. %u), %zu target individuals -> %s\n", S, (base + ".bet").c_str(), its.front(),
                its.back(), nT, out.c_str());
    std::fflush(stdout);
    if (same + swapped == 0) fatal("FATAL  : no marker of " + tp + ".bim matches a training marker (by SNP id and alleles)");

    // target genotypes, read before the device opens
    const size_t lenT = (nT + 3) / 4;
    std::vector<uint8_t> bedT = read_bed(tp, nT, Mt);
    if (opt.predictDryRun) {
        std::printf("PREDICT: dry run: inputs checked, nothing scored\n");
        return 0;
    }

    // the chain's standardisation: mave, mstd of the training markers over the rows that kept their phenotype
    std::vector<double> mave(co.Mtot), mstd(co.Mtot);
    {
        std::vector<uint8_t> bed = read_training(opt.bedFile, co.numInds, co.Mtot);
        hgibbs_t dev = open_training(co, bed);
        hg_check(hgibbs_marker_stats(dev, mave.data(), mstd.data(), nullptr, nullptr, nullptr), "hgibbs_marker_stats");
        hgibbs_destroy(dev);
    }

    hgibbs_t dev = nullptr;
    hg_check(hgibbs_create(co.local_rank, &dev), "hgibbs_create");
    hg_check(hgibbs_load_bed(dev, bedT.data(), lenT, (uint32_t)nT, (uint32_t)Mt, nullptr, 0, (uint32_t)nT, (uint32_t)std::max<size_t>(nT, 2)),
             "hgibbs_load_bed (target)");
    std::vector<uint8_t>().swap(bedT);
    // x = (g - mave) mstd on the chain's scale; a swapped target column counts the other allele: g -> 2 - g
    const size_t chunk = 32;
    std::vector<double> score(nT * S), a, o, part;
    for (size_t s0 = 0; s0 < S; s0 += chunk) {
        const size_t sc = std::min(chunk, S - s0);
        a.assign(sc * Mt, 0.0);
        o.assign(sc * Mt, 0.0);
        for (size_t s = 0; s < sc; ++s) {
            const double* b = betas.data() + (s0 + s) * co.Mtot;
            for (size_t t = 0; t < Mt; ++t) {
                if (match[t] < 0) continue;
                const unsigned j = (unsigned)match[t];
                const double w = b[j] * mstd[j];
                a[s * Mt + t] = flip[t] ? -w : w;
                o[s * Mt + t] = flip[t] ? w * (2.0 - mave[j]) : -w * mave[j];
            }
        }
        part.resize(nT * sc);
        hg_check(hgibbs_score(dev, (int)sc, a.data(), o.data(), part.data()), "hgibbs_score");
        for (size_t i = 0; i < nT; ++i)
            for (size_t s = 0; s < sc; ++s) score[i * S + s0 + s] = part[i * sc + s];
    }
    hgibbs_destroy(dev);

    FILE* f = open_out(out, "w");
    std::fprintf(f, "FID IID mean sd\n");
    for (size_t i = 0; i < nT; ++i) {
        double m = 0.0;
        for (size_t s = 0; s < S; ++s) m += score[i * S + s];
        m /= (double)S;
        double v = 0.0;
        for (size_t s = 0; s < S; ++s) v += (score[i * S + s] - m) * (score[i * S + s] - m);
        const double sd = S > 1 ? std::sqrt(v / (double)(S - 1)) : 0.0;
        std::fprintf(f, "%s %s %.17g %.17g\n", tfam.fid[i].c_str(), tfam.iid[i].c_str(), m, sd);
    }
    close_out(f, out);
    f = open_out(out + ".bin", "wb");
    const uint32_t hdr[2] = {(uint32_t)nT, (uint32_t)S};
    pwrite_at(f, 0, hdr, sizeof hdr);
    pwrite_at(f, sizeof hdr, score.data(), score.size() * sizeof(double));
    close_out(f, out + ".bin");
    std::printf("PREDICT: wrote %s and %s.bin\n", out.c_str(), out.c_str());
    return 0;
}

// ---- --ld-window: windowed LD of the training markers on the chain's rows ----
int run_ld(const Options& opt, const Cohort& co)
{
    const std::string out = opt.ldOut.empty() ? opt.mcmcOutDir + "/" + opt.mcmcOutNam + ".ld" : opt.ldOut;
    const BimRows bim = read_bim(opt.bedFile + ".bim", co.Mtot);
    const uint32_t W = (uint32_t)opt.ldWindow;
    const long long maxbp = opt.ldKbGiven ? (long long)std::llround(1000.0 * opt.ldWindowKb) : -1;
    // a pair (j, q) is kept when 0 < q - j <= W in .bim order, on one chromosome and, with --ld-window-kb, within 1000 KB bp
    auto kept = [&](unsigned j, unsigned q) {
        return bim.chr[q] == bim.chr[j] && (maxbp < 0 || std::llabs(bim.bp[q] - bim.bp[j]) <= maxbp);
    };
    std::map<std::string, int> chroms;
    unsigned long long npairs = 0;
    for (unsigned j = 0; j < co.Mtot; ++j) {
        chroms.emplace(bim.chr[j], 1);
        for (unsigned q = j + 1; q < co.Mtot && q - j <= W; ++q) npairs += kept(j, q) ? 1u : 0u;
    }
    std::printf("LD     : %u markers, window %u markers%s, %zu chromosomes, %llu pairs in the window; r^2 >= %g -> %s%s\n", co.Mtot, W,
                maxbp >= 0 ? (" and " + std::to_string(maxbp) + " bp").c_str() : "", chroms.size(), npairs, opt.ldWindowR2, out.c_str(),
                opt.ldBin ? (" and " + out + ".bin").c_str() : "");
    std::fflush(stdout);

    std::vector<uint8_t> bed = read_training(opt.bedFile, co.numInds, co.Mtot);
    if (opt.ldOut.empty()) make_out_dir(opt);
    FILE* f = open_out(out, "w");
    FILE* fb = nullptr;
    if (opt.ldBin) {
        fb = open_out(out + ".bin", "wb");
        const uint32_t hdr[2] = {co.Mtot, W};
        if (std::fwrite(hdr, sizeof hdr, 1, fb) != 1) fatal("FATAL  : short write on " + out + ".bin");
    }
    std::fprintf(f, "CHR_A BP_A SNP_A CHR_B BP_B SNP_B R\n");

    // the chain's rows and its standardisation
    hgibbs_t dev = open_training(co, bed);
    hg_check(hgibbs_marker_stats(dev, nullptr, nullptr, nullptr, nullptr, nullptr), "hgibbs_marker_stats");

    // chunks of markers: host memory stays at about 2^22 pairs
    const unsigned chunk = std::max(1u, (unsigned)((1u << 22) / W));
    std::vector<double> r;
    std::vector<float> rf;
    unsigned long long written = 0;
    double ms = 0.0;
    for (unsigned m0 = 0; m0 < co.Mtot; m0 += chunk) {
        const unsigned cnt = std::min(chunk, co.Mtot - m0);
        r.resize((size_t)cnt * W);
        hg_check(hgibbs_ld(dev, m0, cnt, W, r.data(), nullptr), "hgibbs_ld");
        double t = 0.0;
        hg_check(hgibbs_last_ld_ms(dev, &t), "hgibbs_last_ld_ms");
        ms += t;
        if (fb) rf.assign((size_t)cnt * W, std::numeric_limits<float>::quiet_NaN());
        for (unsigned jj = 0; jj < cnt; ++jj) {
            const unsigned j = m0 + jj;
            for (unsigned d = 1; d <= W && j + d < co.Mtot; ++d) {
                const unsigned q = j + d;
                const double v = r[(size_t)jj * W + d - 1];
                if (std::isnan(v) || !kept(j, q)) continue;
                if (fb) rf[(size_t)jj * W + d - 1] = (float)v;
                if (v * v < opt.ldWindowR2) continue;
                std::fprintf(f, "%s %lld %s %s %lld %s %.12g\n", bim.chr[j].c_str(), bim.bp[j], bim.id[j].c_str(), bim.chr[q].c_str(), bim.bp[q],
                             bim.id[q].c_str(), v);
                ++written;
            }
        }
        if (fb && std::fwrite(rf.data(), sizeof(float), rf.size(), fb) != rf.size()) fatal("FATAL  : short write on " + out + ".bin");
    }
    hgibbs_destroy(dev);
    close_out(f, out);
    if (fb) close_out(fb, out + ".bin");
    std::printf("LD     : wrote %llu pairs with r^2 >= %g to %s (%.3f ms on the device)\n", written, opt.ldWindowR2, out.c_str(), ms);
    return 0;
}

// ---- --assoc: per-marker association tests with LOCO offsets ----
// Z'Z = L L' (Cholesky, in place, lower triangle); false when Z is rank-deficient
bool cholesky(std::vector<double>& A, int q)
{
    for (int k = 0; k < q; ++k) {
        const double d0 = A[(size_t)k * q + k];
        double d = d0;
        for (int p = 0; p < k; ++p) d -= A[(size_t)k * q + p] * A[(size_t)k * q + p];
        if (!(d > 1e-12 * d0)) return false;
        d = std::sqrt(d);
        A[(size_t)k * q + k] = d;
        for (int i = k + 1; i < q; ++i) {
            double v = A[(size_t)i * q + k];
            for (int p = 0; p < k; ++p) v -= A[(size_t)i * q + p] * A[(size_t)k * q + p];
            A[(size_t)i * q + k] = v / d;
        }
    }
    return true;
}

// x = (L L')^-1 b
std::vector<double> chol_solve(const std::vector<double>& L, int q, std::vector<double> b)
{
    for (int i = 0; i < q; ++i) {
        for (int p = 0; p < i; ++p) b[i] -= L[(size_t)i * q + p] * b[p];
        b[i] /= L[(size_t)i * q + i];
    }
    for (int i = q - 1; i >= 0; --i) {
        for (int p = i + 1; p < q; ++p) b[i] -= L[(size_t)p * q + i] * b[p];
        b[i] /= L[(size_t)i * q + i];
    }
    return b;
}

// the chain's scaling of a phenotype (hydra_chain.cpp): centre, then y'y = N - 1
void scale_phenotype(std::vector<double>& y, unsigned N)
{
    double mean = 0.0;
    for (unsigned i = 0; i < N; ++i) mean += y[i];
    mean /= N;
    for (unsigned i = 0; i < N; ++i) y[i] -= mean;
    double sqn = 0.0;
    for (unsigned i = 0; i < N; ++i) sqn += y[i] * y[i];
    sqn = std::sqrt((double)(N - 1) / sqn);
    for (unsigned i = 0; i < N; ++i) y[i] *= sqn;
}

// Z = [1 | covariates] over N rows and the projection off its columns, for --assoc and --he (`flag`: who refuses dependent columns)
struct CovProjector {
    unsigned N;
    int q;
    std::vector<double> Z; // column-major: Z[c * N + i]
    std::vector<double> L; // the Cholesky factor of Z'Z
    CovProjector(const char* flag, const std::vector<double>& covX, int C, unsigned N_) : N(N_), q(1 + C), Z((size_t)(1 + C) * N_), L((size_t)(1 + C) * (1 + C))
    {
        for (unsigned i = 0; i < N; ++i) {
            Z[i] = 1.0;
            for (int c = 0; c < C; ++c) Z[(size_t)(1 + c) * N + i] = covX[(size_t)i * C + c];
        }
        for (int a = 0; a < q; ++a)
            for (int b = 0; b < q; ++b) {
                double v = 0.0;
                for (unsigned i = 0; i < N; ++i) v += Z[(size_t)a * N + i] * Z[(size_t)b * N + i];
                L[(size_t)a * q + b] = v;
            }
        if (!cholesky(L, q)) fatal(std::string("FATAL  : ") + flag + ": the covariates are rank-deficient (Z = [1 | covariates] has dependent columns)");
    }
    void project(std::vector<double>& v) const // v <- v - Z (Z'Z)^-1 Z'v
    {
        std::vector<double> w(q, 0.0);
        for (int a = 0; a < q; ++a)
            for (unsigned i = 0; i < N; ++i) w[a] += Z[(size_t)a * N + i] * v[i];
        w = chol_solve(L, q, w);
        for (int a = 0; a < q; ++a)
            for (unsigned i = 0; i < N; ++i) v[i] -= Z[(size_t)a * N + i] * w[a];
    }
};

// maximal runs of equal chromosome in .bim order (an unsorted .bim works); chromosome c(j) as an index
struct ChromRuns {
    std::vector<int> cj;
    std::vector<unsigned> runs; // first marker of each run, then Mtot
    size_t nruns = 0, nchrom = 0;
    ChromRuns(const BimRows& bim, unsigned Mtot) : cj(Mtot)
    {
        std::map<std::string, int> chrom_idx;
        for (unsigned j = 0; j < Mtot; ++j) {
            cj[j] = chrom_idx.emplace(bim.chr[j], (int)chrom_idx.size()).first->second;
            if (j == 0 || bim.chr[j] != bim.chr[j - 1]) runs.push_back(j);
        }
        nruns = runs.size();
        nchrom = chrom_idx.size();
        runs.push_back(Mtot);
    }
};

// What both models of --assoc share.  The constructor: the names, the .bim and its runs, the chain's records for LOCO, the banner, the
// refusals of too few rows and of dependent covariates.  open(), after the model's own refusals: the genotypes, the table, the device
// with the chain's rows, the marker statistics.
struct AssocFrame {
    const Options& opt;
    const Cohort& co;
    const std::string base, out;
    const bool loco;
    const BimRows bim;
    const unsigned N;
    const int C, q;
    const ChromRuns cr;
    std::vector<unsigned> its;
    std::vector<double> betas, mave, mstd;
    std::vector<uint64_t> n1, n2, nmiss;
    std::optional<CovProjector> proj; // Z = [1 | covariates]
    FILE* f = nullptr;
    hgibbs_t dev = nullptr;
    double ms = 0.0; // device time of the tests
    unsigned long long written = 0;

    AssocFrame(const Options& opt_, const Cohort& co_, const std::vector<double>& covX, int C_, bool logistic)
        : opt(opt_), co(co_), base(opt_.mcmcOutDir + "/" + opt_.mcmcOutNam), out(opt_.assocOut.empty() ? base + (logistic ? ".assoc.logistic" : ".assoc") : opt_.assocOut), loco(!opt_.assocNoLoco),
          bim(read_bim(opt_.bedFile + ".bim", co_.Mtot)), N(co_.Ntot), C(C_), q(1 + C_), cr(bim, co_.Mtot), mave(co_.Mtot), mstd(co_.Mtot), n1(co_.Mtot), n2(co_.Mtot),
          nmiss(co_.Mtot)
    {
        if (loco) read_bet_records(base + ".bet", co.Mtot, opt.burnin, its, betas, "--assoc takes its LOCO offsets from the chain's effects");
        std::printf("ASSOC  : %u markers, %zu chromosomes in %zu runs, %d covariates, %u individuals -> %s\n", co.Mtot, cr.nchrom, cr.nruns, C, N, out.c_str());
        if (loco)
            std::printf("ASSOC  : LOCO %s from %zu records of %s (iterations %u .. %u)\n", logistic ? "predictors" : "offsets", its.size(), (base + ".bet").c_str(), its.front(), its.back());
        else
            std::printf("ASSOC  : %s\n", logistic ? "no LOCO predictor (--assoc-no-loco): one null model of [1 | covariates] for every chromosome"
                                              : "no LOCO offsets (--assoc-no-loco): every chromosome is tested against the scaled phenotype");
        if (loco && cr.nchrom == 1) std::printf("WARNING: --assoc with one chromosome: G - G_c is 0, no offset is taken out\n");
        std::fflush(stdout);
        if ((long long)N <= (long long)q + 1) fatal("FATAL  : --assoc needs more individuals (" + std::to_string(N) + ") than covariates + 2");
        proj.emplace("--assoc", covX, C, N);
    }

    void open(const std::string& header)
    {
        std::vector<uint8_t> bed = read_training(opt.bedFile, co.numInds, co.Mtot);
        if (opt.assocOut.empty()) make_out_dir(opt);
        f = open_out(out, "w");
        std::fprintf(f, "%s\n", header.c_str());
        dev = open_training(co, bed); // the chain's rows and standardisation
        hg_check(hgibbs_marker_stats(dev, mave.data(), mstd.data(), n1.data(), n2.data(), nmiss.data()), "hgibbs_marker_stats");
    }

    // gc[c][i] = G - G_c, the chain's genetic value of row i without chromosome c.  G_c: the mean effects of the .bet records through
    // hgibbs_score with one "sample" per chromosome; its device time is added to ms
    std::vector<std::vector<double>> loco_predictors()
    {
        const unsigned Mtot = co.Mtot;
        const size_t S = its.size(), nchrom = cr.nchrom;
        std::vector<double> bbar(Mtot, 0.0);
        for (size_t s = 0; s < S; ++s)
            for (unsigned j = 0; j < Mtot; ++j) bbar[j] += betas[s * Mtot + j];
        for (unsigned j = 0; j < Mtot; ++j) bbar[j] /= (double)S;
        std::vector<double> a(nchrom * Mtot, 0.0), o(nchrom * Mtot, 0.0), Gc((size_t)N * nchrom);
        for (unsigned j = 0; j < Mtot; ++j) {
            if (!std::isfinite(mstd[j])) continue; // (score refuses non-finite weights; x = 0 there anyway)
            a[(size_t)cr.cj[j] * Mtot + j] = bbar[j] * mstd[j];
            o[(size_t)cr.cj[j] * Mtot + j] = -bbar[j] * mstd[j] * mave[j];
        }
        hg_check(hgibbs_score(dev, (int)nchrom, a.data(), o.data(), Gc.data()), "hgibbs_score");
        add_ms(hgibbs_last_score_ms, "hgibbs_last_score_ms", ms);
        std::vector<std::vector<double>> gc(nchrom, std::vector<double>(N));
        for (unsigned i = 0; i < N; ++i) {
            double G = 0.0;
            for (size_t c = 0; c < nchrom; ++c) G += Gc[(size_t)i * nchrom + c];
            for (size_t c = 0; c < nchrom; ++c) gc[c][i] = G - Gc[(size_t)i * nchrom + c];
        }
        return gc;
    }

    void add_ms(int (*last)(hgibbs_t, double*), const char* what, double& total) const // the device time of the last call of an operator
    {
        double t = 0.0;
        hg_check(last(dev, &t), what);
        total += t;
    }
    void close()
    {
        hgibbs_destroy(dev);
        close_out(f, out);
    }
    unsigned long long called(unsigned j) const { return (unsigned long long)N - nmiss[j]; }
    void row_prefix(unsigned j) const // CHR SNP BP A1 A2 FREQ N of marker j, and the blank before the model's columns
    {
        std::fprintf(f, "%s %s %lld %s %s %.12g %llu ", bim.chr[j].c_str(), bim.id[j].c_str(), bim.bp[j], bim.a1[j].c_str(), bim.a2[j].c_str(), mave[j] / 2.0, called(j));
    }
};

int run_assoc(const Options& opt, const Cohort& co, const std::vector<double>& y_raw, const std::vector<double>& covX, int C)
{
    AssocFrame fr(opt, co, covX, C, false);
    const unsigned N = fr.N;
    const int q = fr.q, K = 1 + q;
    std::vector<double> y(y_raw); // the chain's scaled phenotype
    scale_phenotype(y, N);
    fr.open("CHR SNP BP A1 A2 FREQ N BETA SE CHISQ P");

    // r_c = y - (G - G_c), projected off Z
    std::vector<std::vector<double>> r(fr.loco ? fr.cr.nchrom : 1, y);
    if (fr.loco) {
        const std::vector<std::vector<double>> gc = fr.loco_predictors();
        for (size_t c = 0; c < r.size(); ++c)
            for (unsigned i = 0; i < N; ++i) r[c][i] = y[i] - gc[c][i];
    }
    std::vector<double> rr(r.size(), 0.0);
    for (size_t c = 0; c < r.size(); ++c) {
        fr.proj->project(r[c]);
        for (unsigned i = 0; i < N; ++i) rr[c] += r[c][i] * r[c][i];
    }

    // one hgibbs_marker_dots per run: U = [r_c, columns of Z] gives s = x_j'r_c and t = Z'x_j
    std::vector<double> U((size_t)K * N), dots;
    std::copy(fr.proj->Z.begin(), fr.proj->Z.end(), U.begin() + N);
    const double dof = (double)N - (double)q - 1.0;
    for (size_t ru = 0; ru < fr.cr.nruns; ++ru) {
        const unsigned m0 = fr.cr.runs[ru], cnt = fr.cr.runs[ru + 1] - fr.cr.runs[ru];
        const size_t c = fr.loco ? (size_t)fr.cr.cj[m0] : 0;
        std::copy(r[c].begin(), r[c].end(), U.begin());
        dots.resize((size_t)cnt * K);
        hg_check(hgibbs_marker_dots(fr.dev, m0, cnt, K, U.data(), dots.data(), nullptr), "hgibbs_marker_dots");
        fr.add_ms(hgibbs_last_marker_dots_ms, "hgibbs_last_marker_dots_ms", fr.ms);
        for (unsigned jj = 0; jj < cnt; ++jj) {
            const unsigned j = m0 + jj;
            const double m = fr.mave[j], sd = fr.mstd[j];
            const double n0 = (double)(fr.called(j) - fr.n1[j] - fr.n2[j]);
            const double xx = sd * sd * ((double)fr.n1[j] * (1.0 - m) * (1.0 - m) + (double)fr.n2[j] * (2.0 - m) * (2.0 - m) + n0 * m * m);
            const double s = dots[(size_t)jj * K];
            std::vector<double> tz(dots.begin() + (size_t)jj * K + 1, dots.begin() + (size_t)(jj + 1) * K);
            const std::vector<double> w = chol_solve(fr.proj->L, q, tz);
            double v = xx;
            for (int a = 0; a < q; ++a) v -= tz[a] * w[a];
            fr.row_prefix(j);
            if (!std::isfinite(sd) || !(v > 1e-9 * xx)) std::fprintf(fr.f, "NA NA NA NA\n");
            else {
                const double b = s / v;
                const double s2 = (rr[c] - s * s / v) / dof;
                const double se = std::sqrt(s2 / v);
                const double chisq = b * b / (se * se);
                std::fprintf(fr.f, "%.12g %.12g %.12g %.12g\n", b * sd, se * sd, chisq, std::erfc(std::sqrt(chisq / 2.0)));
            }
            ++fr.written;
        }
    }
    fr.close();
    std::printf("ASSOC  : wrote %llu rows to %s (%.3f ms on the device)\n", fr.written, fr.out.c_str(), fr.ms);
    return 0;
}

// The two values of a case/control phenotype on the kept rows, ascending (the larger one is the case); anything else is refused in
// the name of the mode `flag` (--assoc-logistic, --epistasis)
std::vector<double> case_control_values(const char* flag, const std::vector<double>& y_raw, unsigned N)
{
    std::vector<double> vals(y_raw.begin(), y_raw.begin() + N);
    std::sort(vals.begin(), vals.end());
    vals.erase(std::unique(vals.begin(), vals.end()), vals.end());
    if (vals.size() != 2)
        fatal(std::string("FATAL  : ") + flag + ": the phenotype takes " + std::to_string(vals.size()) +
              " distinct values on the kept rows, a case/control phenotype takes exactly two (the larger one is the case)");
    return vals;
}

// ---- --assoc --assoc-logistic: the logistic score test of a case/control phenotype ----
struct LogitNull {
    std::vector<double> coef, mu, w, L;
    int iters = 0;
};

// The null models: the case indicator d, the columns Zc = [1 | covariates | the run's LOCO predictor] and one fit per chromosome (one in
// all without a predictor column).  The constructor holds the mode's refusals, which come before any device call.
struct LogitNulls {
    const unsigned N;
    const int q;
    const bool gcol;   // the LOCO predictor G - G_c as a column of the null model
    const int qn, K;   // columns of the null model; vectors of a run: y - mu, w z_1 .. w z_qn, the case indicator
    std::vector<double> d, Zc, U;
    unsigned ncase = 0;
    std::vector<LogitNull> nulls;
    std::vector<std::vector<double>> gc; // the last column per chromosome
    int iters = 0;

    LogitNulls(const AssocFrame& fr, const std::vector<double>& y_raw)
        : N(fr.N), q(fr.q), gcol(fr.loco && fr.cr.nchrom > 1), qn(q + (gcol ? 1 : 0)), K(2 + qn), d(fr.N), Zc((size_t)qn * fr.N), U((size_t)K * fr.N)
    {
        const std::vector<double> vals = case_control_values("--assoc-logistic", y_raw, N);
        if (K > 32)
            fatal("FATAL  : --assoc-logistic: " + std::to_string(fr.C) + " covariates make " + std::to_string(K) + " vectors (y - mu, one per column of the null model" +
                  (gcol ? " with the LOCO predictor" : "") + ", the case indicator), hgibbs_marker_class_sums takes at most 32");
        for (unsigned i = 0; i < N; ++i) ncase += (d[i] = y_raw[i] == vals[1] ? 1.0 : 0.0) != 0.0;
        std::copy(fr.proj->Z.begin(), fr.proj->Z.end(), Zc.begin());
        nulls.resize(gcol ? fr.cr.nchrom : 1);
        fit(q, nulls[0]); // (with a LOCO predictor this one only refuses early; the fits per chromosome follow)
        iters = gcol ? 0 : nulls[0].iters;
        std::copy(d.begin(), d.end(), U.begin() + (size_t)(K - 1) * N);
    }
    void fit(int cols, LogitNull& f)
    {
        f = LogitNull{std::vector<double>(cols), std::vector<double>(N), std::vector<double>(N), std::vector<double>((size_t)cols * cols), 0};
        hg_check(hgibbs_logit_null(N, cols, Zc.data(), d.data(), f.coef.data(), f.mu.data(), f.w.data(), f.L.data(), &f.iters), "--assoc-logistic");
    }
    // one null model per chromosome on [1 | covariates | G - G_c]: the predictor is on the scaled phenotype's scale and gets a coefficient
    void fit_chromosomes(AssocFrame& fr)
    {
        if (gcol) gc = fr.loco_predictors();
        for (size_t c = 0; c < gc.size(); ++c) {
            std::copy(gc[c].begin(), gc[c].end(), Zc.begin() + (size_t)q * N);
            fit(qn, nulls[c]);
            iters += nulls[c].iters;
        }
    }
    // The null model of the run that starts at marker m0; Zc and U = [y - mu, w z_1 .. w z_qn, d] become that run's
    const LogitNull& begin_run(const AssocFrame& fr, unsigned m0)
    {
        const size_t c = gcol ? (size_t)fr.cr.cj[m0] : 0;
        const LogitNull& nm = nulls[c];
        if (gcol) std::copy(gc[c].begin(), gc[c].end(), Zc.begin() + (size_t)q * N);
        for (unsigned i = 0; i < N; ++i) {
            U[i] = d[i] - nm.mu[i];
            for (int a = 0; a < qn; ++a) U[(size_t)(1 + a) * N + i] = nm.w[i] * Zc[(size_t)a * N + i];
        }
        return nm;
    }
};

// --assoc-sets: the file, the weights' parameters and the sets' places, each refused before any device call; then what the runs keep per
// member for the sets' tests, and the results
struct SetPlan {
    const bool on;
    const std::string out;
    MarkerSets msets;
    double a = 1.0, b = 25.0, maf = 0.5;
    std::vector<long> mem_at;         // per marker: its slot among the sets' members, or -1
    std::vector<size_t> set_run;      // per set: the run of its markers (nruns: none of its ids was found)
    std::vector<double> mem_U, mem_v; // per member: its plain score and L^-1 t (qn values)
    std::vector<uint8_t> mem_ok;
    std::vector<hgibbs_set_result> res;
    std::vector<size_t> used; // per set: the members that were tested and pass the MAF bound
    double ms = 0.0;          // device time of hgibbs_set_gram

    SetPlan(const AssocFrame& fr, int qn) : on(!fr.opt.assocSets.empty()), out(fr.opt.assocSetOut.empty() ? fr.base + ".assoc.sets" : fr.opt.assocSetOut)
    {
        if (!on) return;
        const Options& opt = fr.opt;
        size_t unknown = 0, listed = 0, nmem = 0;
        msets = read_sets_file(opt.assocSets, opt.bedFile, fr.bim, fr.co.Mtot, &unknown);
        if (!whole_num(opt.assocSetA, a) || !whole_num(opt.assocSetB, b) || !std::isfinite(a) || !std::isfinite(b) || !(a > 0.0 && b > 0.0))
            fatal("FATAL  : --assoc-set-beta " + opt.assocSetA + " " + opt.assocSetB + ": both parameters of the weights' beta density must be finite numbers > 0");
        if (!whole_num(opt.assocSetMaf, maf) || !std::isfinite(maf) || !(maf > 0.0 && maf <= 0.5))
            fatal("FATAL  : --assoc-set-maf " + opt.assocSetMaf + ": the bound on the minor allele frequency must be a finite number in (0, 0.5]");
        std::vector<size_t> runof(fr.co.Mtot);
        for (size_t ru = 0; ru < fr.cr.nruns; ++ru)
            for (unsigned j = fr.cr.runs[ru]; j < fr.cr.runs[ru + 1]; ++j) runof[j] = ru;
        mem_at.assign(fr.co.Mtot, -1);
        set_run.assign(msets.idx.size(), fr.cr.nruns);
        for (size_t s = 0; s < msets.idx.size(); ++s) {
            const std::vector<uint32_t>& ix = msets.idx[s];
            listed += ix.size();
            for (const uint32_t j : ix) {
                if (runof[j] != runof[ix[0]])
                    fatal("FATAL  : --assoc-sets: set " + msets.name[s] + " has markers on more than one chromosome run (" + fr.bim.id[ix[0]] + " on " + fr.bim.chr[ix[0]] + ", " +
                          fr.bim.id[j] + " on " + fr.bim.chr[j] + "): a set is tested under one null model");
                if (mem_at[j] < 0) mem_at[j] = (long)nmem++;
            }
            if (!ix.empty()) set_run[s] = runof[ix[0]];
        }
        // (the filters need the device's marker statistics, so the operator's limit is held against the ids found: no filter can add one)
        for (size_t s = 0; s < msets.idx.size(); ++s)
            if (msets.idx[s].size() > 1024)
                fatal("FATAL  : --assoc-sets: set " + msets.name[s] + " has " + std::to_string(msets.idx[s].size()) + " markers, hgibbs_set_gram takes at most 1024 a set");
        if (listed == 0)
            fatal("FATAL  : --assoc-sets: none of the " + std::to_string(unknown) + " ids of " + opt.assocSets + " is among the first " + std::to_string(fr.co.Mtot) +
                  " markers of " + opt.bedFile + ".bim");
        std::printf("ASSOC  : %zu sets of %zu markers from %s (%zu ids are not in the .bim), weights dbeta(MAF; %g, %g), MAF <= %g -> %s\n", msets.idx.size(), listed,
                    opt.assocSets.c_str(), unknown, a, b, maf, out.c_str());
        std::fflush(stdout);
        mem_U.assign(nmem, 0.0);
        mem_v.assign(nmem * (size_t)qn, 0.0);
        mem_ok.assign(nmem, 0);
        res.resize(msets.idx.size());
        used.assign(msets.idx.size(), 0);
    }
};

// %.12g, or NA where the number is not defined
std::string num_or_na(double x, bool defined)
{
    char t[32];
    std::snprintf(t, sizeof t, "%.12g", x);
    return defined ? t : "NA";
}

struct AssocRow {
    double beta, se, stat, p;
    int ok; // -2 the marker is not tested (NA); the correction: -1 not applied, 0 applied and fell back to the normal P (the score test), 1 applied and valid
};

// The correction of the score test, --assoc-spa's or --assoc-firth's (never both: check_assoc_args): its threshold, the run's list of
// markers that get it (one entry each, as hgibbs_spa_roots and hgibbs_firth_fit take them), and the counters
struct Correction {
    const bool spa, firth;
    double thr; // --assoc-spa-sd, in standard deviations, or --assoc-firth-p
    std::vector<uint32_t> mk;
    std::vector<double> B, xv, s;
    unsigned long long n = 0, valid = 0;
    double ms = 0.0;
    explicit Correction(const Options& opt) : spa(opt.assocSpa), firth(opt.assocFirth), thr(opt.assocSpa ? 2.0 : 0.05) { whole_num(spa ? opt.assocSpaSd : opt.assocFirthP, thr); }
    bool wants(double U, double V) const // the markers beyond thr standard deviations, resp. whose P is at most thr
    {
        return (spa && std::isfinite(V) && std::fabs(U) / std::sqrt(V) > thr) || (firth && std::isfinite(V) && std::erfc(std::sqrt(U * U / V / 2.0)) <= thr);
    }
};

// The score test of one run: hgibbs_marker_class_sums' sums, and per marker the plain test's row and the row that is written (the plain
// one until correct_run puts a correction's numbers there)
struct RunScores {
    unsigned m0 = 0, cnt = 0;
    std::vector<double> sums, t, v; // t, v: one marker's b_j and L^-1 t
    std::vector<AssocRow> score, row;
    explicit RunScores(int qn) : t(qn), v(qn) {}
};

// One hgibbs_marker_class_sums for the run `ru`, then the score test per marker; a set member's plain score and L^-1 t go to sp, a
// marker that gets a correction to cx's list with b_j = (Z'WZ)^-1 Z'W x_j, the value of each genotype code and the score
void score_run(AssocFrame& fr, const LogitNulls& nl, const LogitNull& nm, size_t ru, RunScores& rs, Correction& cx, SetPlan& sp)
{
    const int qn = nl.qn, K = nl.K;
    const unsigned m0 = rs.m0 = fr.cr.runs[ru], cnt = rs.cnt = fr.cr.runs[ru + 1] - fr.cr.runs[ru];
    std::vector<double>&t = rs.t, &v = rs.v;
    rs.sums.resize((size_t)cnt * K * 4);
    hg_check(hgibbs_marker_class_sums(fr.dev, m0, cnt, K, nl.U.data(), rs.sums.data()), "hgibbs_marker_class_sums");
    fr.add_ms(hgibbs_last_marker_class_sums_ms, "hgibbs_last_marker_class_sums_ms", fr.ms);
    rs.score.assign(cnt, AssocRow{0.0, 0.0, 0.0, 0.0, -2});
    rs.row = rs.score;
    cx.mk.clear();
    cx.B.clear();
    cx.xv.clear();
    cx.s.clear();
    for (unsigned jj = 0; jj < cnt; ++jj) {
        const unsigned j = m0 + jj;
        const double m = fr.mave[j], sd = fr.mstd[j];
        const double* S = &rs.sums[(size_t)jj * K * 4];
        auto xu = [&](int k) { return sd * (S[4 * k + 1] + 2.0 * S[4 * k + 2] - m * (S[4 * k] + S[4 * k + 1] + S[4 * k + 2])); }; // x_j'u_k
        const double xwx = sd * sd * (m * m * S[4] + (1.0 - m) * (1.0 - m) * S[5] + (2.0 - m) * (2.0 - m) * S[6]);
        double V = xwx;
        for (int a = 0; a < qn; ++a) { // v = L^-1 t: t'(Z'WZ)^-1 t = v'v
            double e = xu(1 + a);
            for (int p = 0; p < a; ++p) e -= nm.L[(size_t)a + (size_t)qn * p] * v[p];
            v[a] = e / nm.L[(size_t)a + (size_t)qn * a];
            V -= v[a] * v[a];
        }
        if (!std::isfinite(sd) || !(V > 1e-9 * xwx)) continue;
        const double Uj = xu(0), chisq = Uj * Uj / V;
        rs.row[jj] = rs.score[jj] = {sd * Uj / V, sd / std::sqrt(V), chisq, std::erfc(std::sqrt(chisq / 2.0)), -1};
        if (sp.on && sp.mem_at[j] >= 0) { // a set member keeps its plain score and L^-1 t
            const size_t e = (size_t)sp.mem_at[j];
            sp.mem_ok[e] = 1;
            sp.mem_U[e] = Uj;
            std::copy(v.begin(), v.begin() + qn, sp.mem_v.begin() + e * (size_t)qn);
        }
        if (!cx.wants(Uj, V)) continue;
        for (int a = qn - 1; a >= 0; --a) { // b_j = L^-T v
            double e = v[a];
            for (int p = a + 1; p < qn; ++p) e -= nm.L[(size_t)p + (size_t)qn * a] * t[p];
            t[a] = e / nm.L[(size_t)a + (size_t)qn * a];
        }
        cx.mk.push_back(j);
        cx.B.insert(cx.B.end(), t.begin(), t.end());
        for (const double x : {(0.0 - m) * sd, (1.0 - m) * sd, (2.0 - m) * sd, 0.0}) cx.xv.push_back(x);
        cx.s.push_back(Uj);
    }
}

// The correction of one run: the one device call that applies to cx's list, then per entry the row's four numbers and whether the
// correction holds; where it does not, the entry's row keeps the score test's numbers
void correct_run(AssocFrame& fr, const LogitNulls& nl, const LogitNull& nm, RunScores& rs, Correction& cx)
{
    const uint32_t ne = (uint32_t)cx.mk.size();
    if (ne == 0) return;
    std::vector<hgibbs_spa_root> roots(cx.firth ? 0 : ne);
    std::vector<hgibbs_firth_rec> recs(cx.firth ? ne : 0);
    if (cx.firth) {
        hg_check(hgibbs_firth_fit(fr.dev, ne, cx.mk.data(), nl.qn, nl.Zc.data(), nm.mu.data(), cx.B.data(), cx.xv.data(), cx.s.data(), recs.data()), "hgibbs_firth_fit");
        fr.add_ms(hgibbs_last_firth_ms, "hgibbs_last_firth_ms", cx.ms);
    } else {
        hg_check(hgibbs_spa_roots(fr.dev, ne, cx.mk.data(), nl.qn, nl.Zc.data(), nm.mu.data(), cx.B.data(), cx.xv.data(), cx.s.data(), roots.data()), "hgibbs_spa_roots");
        fr.add_ms(hgibbs_last_spa_ms, "hgibbs_last_spa_ms", cx.ms);
    }
    for (uint32_t e = 0; e < ne; ++e) {
        const double sd = fr.mstd[cx.mk[e]];
        AssocRow& r = rs.row[cx.mk[e] - rs.m0];
        double stat = 0.0, se = 0.0, p = 0.0;
        if (cx.firth) {
            hg_check(hgibbs_firth_stats(cx.s[e], &recs[e], &stat, &se, &p, &r.ok), "hgibbs_firth_stats");
            if (r.ok) r = {sd * recs[e].beta, sd * se, stat, p, r.ok};
        } else {
            hg_check(hgibbs_spa_pvalue(cx.s[e], &roots[e], nullptr, nullptr, &p, &r.ok), "hgibbs_spa_pvalue");
            if (r.ok) r.p = p;
        }
        ++cx.n;
        cx.valid += r.ok ? 1u : 0u;
    }
}

// The rows of one run: the frame's prefix, BETA SE CHISQ P (the correction's where the marker has one), the case/control columns and
// the correction's trailing columns
void write_rows(AssocFrame& fr, int K, const RunScores& rs, const Correction& cx)
{
    for (unsigned jj = 0; jj < rs.cnt; ++jj) {
        const unsigned j = rs.m0 + jj;
        const AssocRow &sc = rs.score[jj], &r = rs.row[jj];
        auto num = [&](double x) { return num_or_na(x, sc.ok > -2); };
        // the sums of the case indicator are exact counts of the cases by genotype; the controls are the rest of the marker's stats
        const double* Sd = &rs.sums[(size_t)jj * K * 4] + 4 * (K - 1);
        const double c1 = Sd[1], c2 = Sd[2], ca = Sd[0] + c1 + c2;
        const double k1 = (double)fr.n1[j] - c1, k2 = (double)fr.n2[j] - c2, ka = (double)fr.called(j) - ca;
        fr.row_prefix(j);
        std::fprintf(fr.f, "%s %s %s %s %.12g %.12g %s %s", num(r.beta).c_str(), num(r.se).c_str(), num(r.stat).c_str(), num(r.p).c_str(), ca, ka,
                     num_or_na((c1 + 2.0 * c2) / (2.0 * ca), ca > 0.0).c_str(), num_or_na((k1 + 2.0 * k2) / (2.0 * ka), ka > 0.0).c_str());
        if (cx.spa || cx.firth) std::fprintf(fr.f, " %s", num(sc.p).c_str()); // P_NORM
        if (cx.firth) std::fprintf(fr.f, " %s %s", num(sc.beta).c_str(), num(sc.se).c_str()); // BETA_SCORE SE_SCORE
        if (cx.spa || cx.firth) std::fprintf(fr.f, " %s", r.ok >= 0 ? std::to_string(r.ok).c_str() : "NA"); // SPA or FIRTH
        std::fprintf(fr.f, "\n");
        ++fr.written;
    }
}

// The sets of the run `ru`: their tested members within the MAF bound, packed into hgibbs_set_gram calls of at most SET_CHUNK entries;
// per set Phi = out - (L^-1 t_j).(L^-1 t_k) with hgibbs_set_gram's out under this run's w, then per copy of A1
void sets_run(const AssocFrame& fr, const LogitNull& nm, int qn, size_t ru, SetPlan& sp)
{
    constexpr uint64_t SET_CHUNK = 1ull << 22; // entries of out per hgibbs_set_gram call (a set of 1024 has 2^20)
    std::vector<size_t> todo;
    for (size_t s = 0; s < sp.msets.idx.size(); ++s)
        if (sp.set_run[s] == ru) todo.push_back(s);
    std::vector<std::vector<uint32_t>> used(todo.size());
    for (size_t k = 0; k < todo.size(); ++k) {
        for (const uint32_t j : sp.msets.idx[todo[k]]) {
            const double p = fr.mave[j] / 2.0;
            if (sp.mem_ok[(size_t)sp.mem_at[j]] && std::min(p, 1.0 - p) <= sp.maf) used[k].push_back(j);
        }
        sp.used[todo[k]] = used[k].size();
    }
    for (size_t k0 = 0; k0 < todo.size();) {
        std::vector<uint64_t> off{0};
        std::vector<uint32_t> gidx;
        std::vector<size_t> part;
        uint64_t E = 0;
        size_t k1 = k0;
        for (; k1 < todo.size(); ++k1) {
            const uint64_t mm = (uint64_t)used[k1].size() * used[k1].size();
            if (!part.empty() && E + mm > SET_CHUNK) break;
            if (mm == 0) continue;
            part.push_back(k1);
            gidx.insert(gidx.end(), used[k1].begin(), used[k1].end());
            off.push_back(gidx.size());
            E += mm;
        }
        k0 = k1;
        if (part.empty()) continue;
        std::vector<double> G(E);
        hg_check(hgibbs_set_gram(fr.dev, (uint32_t)part.size(), off.data(), gidx.data(), nm.w.data(), G.data(), nullptr), "hgibbs_set_gram");
        fr.add_ms(hgibbs_last_set_gram_ms, "hgibbs_last_set_gram_ms", sp.ms);
        uint64_t b0 = 0;
        for (const size_t k : part) {
            const std::vector<uint32_t>& ix = used[k];
            const size_t m = ix.size();
            std::vector<double> Ug(m), Ph(m * m), aw(m);
            const double lc = std::lgamma(sp.a + sp.b) - std::lgamma(sp.a) - std::lgamma(sp.b);
            for (size_t a = 0; a < m; ++a) {
                const size_t ea = (size_t)sp.mem_at[ix[a]];
                const double p = fr.mave[ix[a]] / 2.0, maf = std::min(p, 1.0 - p);
                Ug[a] = sp.mem_U[ea] / fr.mstd[ix[a]];
                aw[a] = std::exp(lc + (sp.a - 1.0) * std::log(maf) + (sp.b - 1.0) * std::log1p(-maf));
                for (size_t b = 0; b < m; ++b) {
                    const size_t eb = (size_t)sp.mem_at[ix[b]];
                    double tt = 0.0;
                    for (int c = 0; c < qn; ++c) tt += sp.mem_v[ea * (size_t)qn + c] * sp.mem_v[eb * (size_t)qn + c];
                    Ph[a * m + b] = (G[b0 + a * m + b] - tt) / (fr.mstd[ix[a]] * fr.mstd[ix[b]]);
                }
            }
            hg_check(hgibbs_set_tests((uint32_t)m, Ug.data(), Ph.data(), aw.data(), &sp.res[todo[k]]), "hgibbs_set_tests");
            b0 += (uint64_t)m * m;
        }
    }
}

void write_sets_table(const BimRows& bim, const SetPlan& sp)
{
    FILE* fs = open_out(sp.out, "w");
    std::fprintf(fs, "SET\tCHR\tBP_FIRST\tBP_LAST\tNSNP\tNUSED\tNEIG\tQ\tP_SKAT\tSKAT_OK\tT_BURDEN\tP_BURDEN\n");
    auto num = [](double x) { return num_or_na(x, std::isfinite(x)); };
    for (size_t s = 0; s < sp.msets.idx.size(); ++s) {
        const std::vector<uint32_t>& ix = sp.msets.idx[s];
        std::fprintf(fs, "%s", sp.msets.name[s].c_str());
        if (ix.empty()) std::fprintf(fs, "\tNA\tNA\tNA");
        else {
            const auto lh = std::minmax_element(ix.begin(), ix.end(), [&](uint32_t a, uint32_t b) { return bim.bp[a] < bim.bp[b]; });
            std::fprintf(fs, "\t%s\t%lld\t%lld", bim.chr[ix[0]].c_str(), bim.bp[*lh.first], bim.bp[*lh.second]);
        }
        std::fprintf(fs, "\t%zu\t%zu", ix.size(), sp.used[s]);
        const hgibbs_set_result& r = sp.res[s];
        if (sp.used[s] == 0) std::fprintf(fs, "\t0\tNA\tNA\tNA\tNA\tNA\n");
        else
            std::fprintf(fs, "\t%d\t%s\t%s\t%s\t%s\t%s\n", r.neig, num(r.q).c_str(), num(r.p_skat).c_str(), r.neig > 0 ? std::to_string(r.skat_ok).c_str() : "NA",
                         num(r.t_burden).c_str(), num(r.p_burden).c_str());
    }
    close_out(fs, sp.out);
}

int run_assoc_logistic(const Options& opt, const Cohort& co, const std::vector<double>& y_raw, const std::vector<double>& covX, int C)
{
    AssocFrame fr(opt, co, covX, C, true);
    LogitNulls nl(fr, y_raw);
    SetPlan sp(fr, nl.qn);
    Correction cx(opt);
    fr.open(std::string("CHR SNP BP A1 A2 FREQ N BETA SE CHISQ P N_CASE N_CTRL FREQ_CASE FREQ_CTRL") +
            (cx.spa ? " P_NORM SPA" : cx.firth ? " P_NORM BETA_SCORE SE_SCORE FIRTH" : ""));
    nl.fit_chromosomes(fr);
    RunScores rs(nl.qn);
    for (size_t ru = 0; ru < fr.cr.nruns; ++ru) {
        const LogitNull& nm = nl.begin_run(fr, fr.cr.runs[ru]);
        score_run(fr, nl, nm, ru, rs, cx, sp);
        correct_run(fr, nl, nm, rs, cx);
        write_rows(fr, nl.K, rs, cx);
        if (sp.on) sets_run(fr, nm, nl.qn, ru, sp);
    }
    fr.close();
    if (sp.on) write_sets_table(fr.bim, sp);
    std::printf("ASSOC  : wrote %llu rows to %s (%u cases, %u controls, %d iterations of %zu null models, %.3f ms on the device)", fr.written, fr.out.c_str(), nl.ncase,
                fr.N - nl.ncase, nl.iters, nl.nulls.size(), fr.ms);
    if (sp.on) std::printf(", %zu sets to %s (%.3f ms of hgibbs_set_gram on the device)", sp.msets.idx.size(), sp.out.c_str(), sp.ms);
    std::printf("\n");
    if (cx.spa || cx.firth)
        std::printf("ASSOC  : %s on %llu markers (%s %g): %llu valid, %llu fell back, %.3f ms on the device\n", cx.spa ? "SPA" : "Firth", cx.n, cx.spa ? "|z| >" : "P <=",
                    cx.thr, cx.valid, cx.n - cx.valid, cx.ms);
    return 0;
}

// ---- --king: KING-robust kinship of the chain's rows ----
int run_king(const Options& opt, const Cohort& co)
{
    const std::string out = opt.kingOut.empty() ? opt.mcmcOutDir + "/" + opt.mcmcOutNam + ".kin0" : opt.kingOut;
    double cutoff = 0.0;
    whole_num(opt.kingCutoff, cutoff);
    // FID and IID of the chain's rows, in .fam order
    const FamIds fam = read_fam_ids(opt.bedFile + ".fam", co.numInds, co.numNAs ? &co.keep : nullptr);
    const unsigned Ntot = co.Ntot;
    if (fam.fid.size() != Ntot) fatal("FATAL  : " + opt.bedFile + ".fam: " + std::to_string(fam.fid.size()) + " kept rows, expected " + std::to_string(Ntot));
    std::vector<uint8_t> bed = read_training(opt.bedFile, co.numInds, co.Mtot);
    if (opt.kingOut.empty()) make_out_dir(opt);
    FILE* f = open_out(out, "w");
    std::fprintf(f, "#FID1\tIID1\tFID2\tIID2\tNSNP\tHETHET\tIBS0\tKINSHIP\n");

    hgibbs_t dev = open_training(co, bed);
    uint64_t np = 0;
    hg_check(hgibbs_king_pairs(dev, cutoff, &np), "hgibbs_king_pairs");
    std::vector<uint32_t> ab(2 * np);
    std::vector<int32_t> cnt(5 * np);
    std::vector<double> kin(np);
    hg_check(hgibbs_king_pairs_get(dev, ab.data(), cnt.data(), kin.data()), "hgibbs_king_pairs_get");
    double ms = 0.0;
    hg_check(hgibbs_last_king_ms(dev, &ms), "hgibbs_last_king_ms");
    hgibbs_destroy(dev);
    // HETHET and IBS0 as proportions of NSNP, as KING's .kin0 writes them; the list comes sorted by (a, b): .fam order
    for (uint64_t p = 0; p < np; ++p) {
        const uint32_t a = ab[2 * p], b = ab[2 * p + 1];
        const int32_t* k = &cnt[5 * p];
        std::fprintf(f, "%s\t%s\t%s\t%s\t%d\t%.12g\t%.12g\t%.12g\n", fam.fid[a].c_str(), fam.iid[a].c_str(), fam.fid[b].c_str(), fam.iid[b].c_str(), k[0],
                     (double)k[3] / (double)k[0], (double)k[4] / (double)k[0], kin[p]);
    }
    close_out(f, out);
    std::printf("KING   : %llu pairs tested, %llu with KINSHIP >= %g written to %s (%.3f ms on the device)\n",
                (unsigned long long)Ntot * (Ntot - 1ull) / 2ull, (unsigned long long)np, cutoff, out.c_str(), ms);
    return 0;
}

// ---- --pca: principal components of the chain's rows ----
constexpr int PCA_KMAX = 24; // the panel is the smallest multiple of 8 that is >= K + 8, at most 32 vectors

int run_pca(const Options& opt, const Cohort& co)
{
    long K = 0, iters = 20;
    double tol = 1e-10;
    whole_int(opt.pcaK, K);
    if (opt.pcaItersGiven) whole_int(opt.pcaIters, iters);
    if (opt.pcaTolGiven) whole_num(opt.pcaTol, tol);
    const int L = std::min(32, (int)((K + 8 + 7) / 8) * 8);
    // <out>: --pca-out without its .eigenvec, else <dir>/<name>
    std::string vec = opt.pcaOut.empty() ? opt.mcmcOutDir + "/" + opt.mcmcOutNam + ".eigenvec" : opt.pcaOut, pre = vec;
    if (pre.size() > 9 && pre.compare(pre.size() - 9, 9, ".eigenvec") == 0) pre.resize(pre.size() - 9);
    // FID and IID of every .fam row; the chain's rows are the kept ones
    const FamIds fam = read_fam_ids(opt.bedFile + ".fam", co.numInds, nullptr);
    if (fam.fid.size() != co.numInds) fatal("FATAL  : " + opt.bedFile + ".fam: " + std::to_string(fam.fid.size()) + " rows, expected " + std::to_string(co.numInds));
    const unsigned Ntot = co.Ntot;
    std::vector<uint8_t> bed = read_training(opt.bedFile, co.numInds, co.Mtot);
    if (opt.pcaOut.empty()) make_out_dir(opt);
    FILE* f = open_out(vec, "w");
    std::fprintf(f, "#FID\tIID");
    for (long k = 0; k < K; ++k) std::fprintf(f, "\tPC%ld", k + 1);
    std::fprintf(f, "\n");
    std::fflush(f);
    std::printf("PCA    : %ld components, panel of %d vectors, at most %ld iterations, tolerance %g, seed %u\n", K, L, iters, tol, opt.seed);

    hgibbs_t dev = open_training(co, bed);
    std::vector<double> eigval(K), pcs((size_t)K * Ntot), load(opt.pcaLoadings ? (size_t)K * co.Mtot : 0);
    hgibbs_pca_report rep;
    hg_check(hgibbs_pca(dev, (int)K, L, (int)iters, tol, nullptr, (uint64_t)opt.seed, eigval.data(), pcs.data(), opt.pcaLoadings ? load.data() : nullptr, &rep),
             "hgibbs_pca");
    double ms[4] = {0, 0, 0, 0};
    hg_check(hgibbs_last_pca_ms(dev, ms), "hgibbs_last_pca_ms");
    hgibbs_destroy(dev);

    FILE* c = open_out(pre + ".cov", "w");
    unsigned at = 0;
    for (unsigned r = 0; r < co.numInds; ++r) {
        const bool kept = !co.numNAs || co.keep[r];
        std::fprintf(c, "%s %s", fam.fid[r].c_str(), fam.iid[r].c_str());
        if (kept) std::fprintf(f, "%s\t%s", fam.fid[r].c_str(), fam.iid[r].c_str());
        for (long k = 0; k < K; ++k) {
            if (kept) {
                std::fprintf(f, "\t%.12g", pcs[(size_t)k * Ntot + at]);
                std::fprintf(c, " %.12g", pcs[(size_t)k * Ntot + at]);
            } else
                std::fprintf(c, " NA");
        }
        std::fprintf(c, "\n");
        if (kept) {
            std::fprintf(f, "\n");
            ++at;
        }
    }
    close_out(f, vec);
    close_out(c, pre + ".cov");
    FILE* v = open_out(pre + ".eigenval", "w");
    for (long k = 0; k < K; ++k) std::fprintf(v, "%.12g\n", eigval[k]);
    close_out(v, pre + ".eigenval");
    if (opt.pcaLoadings) {
        const BimRows bim = read_bim(opt.bedFile + ".bim", co.Mtot);
        FILE* w = open_out(pre + ".var", "w");
        std::fprintf(w, "#CHR\tSNP\tA1\tA2");
        for (long k = 0; k < K; ++k) std::fprintf(w, "\tPC%ld", k + 1);
        std::fprintf(w, "\n");
        for (unsigned j = 0; j < co.Mtot; ++j) {
            std::fprintf(w, "%s\t%s\t%s\t%s", bim.chr[j].c_str(), bim.id[j].c_str(), bim.a1[j].c_str(), bim.a2[j].c_str());
            for (long k = 0; k < K; ++k) {
                const double x = load[(size_t)k * co.Mtot + j];
                if (std::isfinite(x)) std::fprintf(w, "\t%.12g", x);
                else std::fprintf(w, "\tNA");
            }
            std::fprintf(w, "\n");
        }
        close_out(w, pre + ".var");
    }
    double worst = 0.0;
    for (long k = 0; k < K; ++k) worst = std::max(worst, rep.resid[k]);
    std::printf("PCA    : %u rows, %u markers used, panel of %d, %d iterations run, last Ritz change %g, largest residual %g, written to %s (%.3f ms on the device)\n",
                Ntot, rep.m_used, L, rep.iters_run, rep.ritz_change, worst, vec.c_str(), ms[0]);
    return 0;
}

// ---- --pve: posterior variance explained by marker sets ----
struct PveSets : MarkerSets {
    std::string how; // how the sets were defined, for the report
};

PveSets pve_sets(const Options& opt, const BimRows& bim, unsigned Mtot)
{
    PveSets ps;
    auto add = [&](const std::string& name) {
        ps.name.push_back(name);
        ps.idx.emplace_back();
        return ps.idx.size() - 1;
    };
    if (opt.pveKbGiven) {
        double kb = 0.0;
        whole_num(opt.pveKb, kb);
        ps.how = "windows of " + opt.pveKb + " kb";
        std::map<std::pair<std::string, long long>, size_t> at;
        for (unsigned j = 0; j < Mtot; ++j) {
            const long long w = (long long)std::floor((double)bim.bp[j] / (1000.0 * kb));
            auto it = at.find({bim.chr[j], w});
            if (it == at.end()) it = at.emplace(std::make_pair(bim.chr[j], w), add(bim.chr[j] + ":" + std::to_string(w))).first;
            ps.idx[it->second].push_back(j);
        }
    } else if (opt.pveSnpsGiven) {
        long W = 0;
        whole_int(opt.pveSnps, W);
        ps.how = "windows of " + opt.pveSnps + " markers";
        unsigned run0 = 0;
        for (unsigned j = 0; j < Mtot; ++j) {
            if (j && bim.chr[j] != bim.chr[j - 1]) run0 = j;
            if ((j - run0) % (unsigned long)W == 0) {
                unsigned last = j; // the window ends with its run or after W markers
                while (last + 1 < Mtot && last + 1 - j < (unsigned long)W && bim.chr[last + 1] == bim.chr[j]) ++last;
                add(bim.chr[j] + ":" + std::to_string(j + 1) + "-" + std::to_string(last + 1));
            }
            ps.idx.back().push_back(j);
        }
    } else if (!opt.pveSets.empty()) {
        ps.how = "from " + opt.pveSets;
        static_cast<MarkerSets&>(ps) = read_sets_file(opt.pveSets, opt.bedFile, bim, Mtot);
    } else if (opt.pveGroups) {
        ps.how = "the groups of " + opt.groupIndexFile;
        static_cast<MarkerSets&>(ps) = sets_from_groups(opt, Mtot);
    } else {
        ps.how = "one per chromosome";
        std::map<std::string, size_t> at;
        for (unsigned j = 0; j < Mtot; ++j) {
            auto it = at.find(bim.chr[j]);
            if (it == at.end()) it = at.emplace(bim.chr[j], add("chr" + bim.chr[j])).first;
            ps.idx[it->second].push_back(j);
        }
    }
    return ps;
}

int run_pve(const Options& opt, const Cohort& co)
{
    const std::string base = opt.mcmcOutDir + "/" + opt.mcmcOutNam;
    const std::string out = opt.pveOut.empty() ? base + ".pve" : opt.pveOut;
    const unsigned M = co.Mtot, N = co.Ntot;
    const BimRows bim = read_bim(opt.bedFile + ".bim", M);
    PveSets ps = pve_sets(opt, bim, M);
    const size_t nsets = ps.idx.size();
    std::vector<unsigned> its;
    std::vector<double> betas;
    read_bet_records(base + ".bet", M, opt.burnin, its, betas, "--pve takes the variance explained from the chain's effects");
    const size_t S = its.size();
    double T = 1.0 / (double)nsets;
    if (opt.pveThresholdGiven) whole_num(opt.pveThreshold, T);
    std::printf("PVE    : %zu sets (%s), %u markers, %u individuals, %zu records of %s (iterations %u .. %u), threshold %g -> %s\n", nsets, ps.how.c_str(), M,
                N, S, (base + ".bet").c_str(), its.front(), its.back(), T, out.c_str());
    std::fflush(stdout);
    if (N < 2) fatal("FATAL  : --pve needs at least two individuals");

    // the last set: every marker
    ps.name.push_back("ALL");
    ps.idx.emplace_back(M);
    for (unsigned j = 0; j < M; ++j) ps.idx.back()[j] = j;
    const size_t R = nsets + 1;
    std::vector<uint64_t> off(R + 1, 0);
    for (size_t r = 0; r < R; ++r) off[r + 1] = off[r] + ps.idx[r].size();
    std::vector<uint32_t> idx;
    idx.reserve(off[R]);
    for (const auto& r : ps.idx) idx.insert(idx.end(), r.begin(), r.end());

    std::vector<uint8_t> bed = read_training(opt.bedFile, co.numInds, M);
    if (opt.pveOut.empty()) make_out_dir(opt);
    FILE* f = open_out(out, "w");
    std::fprintf(f, "SET CHR BP_FIRST BP_LAST NSNP PIP PVE_MEAN PVE_SD SHARE_MEAN SHARE_SD WPPA\n");
    FILE* fb = opt.pveBin ? open_out(out + ".bin", "wb") : nullptr;

    // the chain's rows and standardisation; the records in chunks of at most 32
    hgibbs_t dev = open_training(co, bed);
    std::vector<double> mave(M), mstd(M);
    hg_check(hgibbs_marker_stats(dev, mave.data(), mstd.data(), nullptr, nullptr, nullptr), "hgibbs_marker_stats");
    std::vector<double> var(R * S); // set-major
    double ms = 0.0;
    const size_t CH = 32;
    std::vector<double> a(CH * M), o(CH * M), mean(R * CH), v(R * CH);
    for (size_t s0 = 0; s0 < S; s0 += CH) {
        const size_t ns = std::min(CH, S - s0);
        for (size_t s = 0; s < ns; ++s)
            for (unsigned j = 0; j < M; ++j) {
                const double b = betas[(s0 + s) * M + j];
                const bool live = b != 0.0 && std::isfinite(mstd[j]);
                a[s * M + j] = live ? b * mstd[j] : 0.0;
                o[s * M + j] = live ? -b * mstd[j] * mave[j] : 0.0;
            }
        hg_check(hgibbs_region_var(dev, (int)ns, a.data(), o.data(), (uint32_t)R, off.data(), idx.data(), mean.data(), v.data()), "hgibbs_region_var");
        double t = 0.0;
        hg_check(hgibbs_last_region_var_ms(dev, &t), "hgibbs_last_region_var_ms");
        ms += t;
        for (size_t r = 0; r < R; ++r)
            for (size_t s = 0; s < ns; ++s) var[r * S + s0 + s] = v[r * ns + s];
    }
    hgibbs_destroy(dev);

    if (fb) {
        const uint32_t hd[2] = {(uint32_t)R, (uint32_t)S};
        if (std::fwrite(hd, sizeof(uint32_t), 2, fb) != 2 || std::fwrite(var.data(), sizeof(double), var.size(), fb) != var.size())
            fatal("FATAL  : short write on " + out + ".bin");
        close_out(fb, out + ".bin");
    }
    auto num = [&](double x, bool na) {
        if (na) std::fprintf(f, " NA");
        else std::fprintf(f, " %.12g", x);
    };
    auto mean_sd = [&](const std::vector<double>& x, double& m, double& sd) {
        m = 0.0;
        for (double y : x) m += y;
        m /= (double)x.size();
        sd = 0.0;
        for (double y : x) sd += (y - m) * (y - m);
        sd = x.size() > 1 ? std::sqrt(sd / (double)(x.size() - 1)) : 0.0;
    };
    std::vector<double> pve(S), share(S);
    for (size_t r = 0; r < R; ++r) {
        const std::vector<uint32_t>& set = ps.idx[r];
        bool one_chr = !set.empty();
        long long bp0 = 0, bp1 = 0;
        for (size_t k = 0; k < set.size(); ++k) {
            const uint32_t j = set[k];
            if (bim.chr[j] != bim.chr[set[0]]) one_chr = false;
            bp0 = k ? std::min(bp0, bim.bp[j]) : bim.bp[j];
            bp1 = k ? std::max(bp1, bim.bp[j]) : bim.bp[j];
        }
        size_t nin = 0, nabove = 0;
        for (size_t s = 0; s < S; ++s) {
            bool in = false;
            for (const uint32_t j : set)
                if (betas[s * M + j] != 0.0) {
                    in = true;
                    break;
                }
            nin += in;
            const double all = var[nsets * S + s];
            pve[s] = var[r * S + s];
            share[s] = all != 0.0 ? pve[s] / all : 0.0;
            nabove += share[s] > T;
        }
        double pm, psd, sm, ssd;
        mean_sd(pve, pm, psd);
        mean_sd(share, sm, ssd);
        std::fprintf(f, "%s", ps.name[r].c_str());
        if (one_chr) std::fprintf(f, " %s %lld %lld", bim.chr[set[0]].c_str(), bp0, bp1);
        else std::fprintf(f, " NA NA NA");
        std::fprintf(f, " %zu", set.size());
        num((double)nin / (double)S, false);
        num(pm, false);
        num(psd, S < 2);
        num(sm, false);
        num(ssd, S < 2);
        num((double)nabove / (double)S, false);
        std::fprintf(f, "\n");
    }
    close_out(f, out);
    std::printf("PVE    : wrote %zu rows to %s (%.3f ms on the device)\n", R, out.c_str(), ms);
    return 0;
}

// ---- --grm: genomic relationship matrix of the chain's rows ----
int run_grm(const Options& opt, const Cohort& co)
{
    const std::string prefix = opt.grmOut.empty() ? opt.mcmcOutDir + "/" + opt.mcmcOutNam : opt.grmOut;
    double T = 0.0;
    if (opt.grmSparseGiven) whole_num(opt.grmSparse, T);
    const FamIds fam = read_fam_ids(opt.bedFile + ".fam", co.numInds, co.numNAs ? &co.keep : nullptr);
    const unsigned N = co.Ntot;
    if (fam.fid.size() != N) fatal("FATAL  : " + opt.bedFile + ".fam: " + std::to_string(fam.fid.size()) + " kept rows, expected " + std::to_string(N));
    std::vector<uint8_t> bed = read_training(opt.bedFile, co.numInds, co.Mtot);
    if (opt.grmOut.empty()) make_out_dir(opt);
    const std::string idp = prefix + ".grm.id", binp = prefix + ".grm.bin", nbinp = prefix + ".grm.N.bin", spp = prefix + ".grm.sp";
    FILE* fid = open_out(idp, "w");
    for (unsigned i = 0; i < N; ++i) std::fprintf(fid, "%s\t%s\n", fam.fid[i].c_str(), fam.iid[i].c_str());
    close_out(fid, idp);
    FILE* fb = open_out(binp, "wb");
    FILE* fn = open_out(nbinp, "wb");
    FILE* fs = opt.grmSparseGiven ? open_out(spp, "w") : nullptr;

    hgibbs_t dev = open_training(co, bed);
    // rows in chunks: at most 2^25 pairs (what the device holds at a time) and, with the f32 copies, a quarter of the free host memory
    const long pages = sysconf(_SC_AVPHYS_PAGES), psz = sysconf(_SC_PAGESIZE);
    const unsigned long long avail = pages > 0 && psz > 0 ? (unsigned long long)pages * (unsigned long long)psz : (1ull << 30);
    const unsigned long long cap = std::max<unsigned long long>(1, std::min<unsigned long long>(1ull << 25, avail / 4 / 20));
    std::vector<double> S;
    std::vector<int32_t> ns;
    std::vector<float> fa, fc;
    double ms = 0.0;
    unsigned long long pairs = 0, above = 0;
    uint32_t used = 0;
    for (unsigned a0 = 0; a0 < N;) {
        unsigned a1 = a0;
        unsigned long long n = 0;
        while (a1 < N && (a1 == a0 || n + a1 + 1ull <= cap)) n += a1++ + 1ull;
        S.resize(n);
        ns.resize(n);
        fa.resize(n);
        fc.resize(n);
        hg_check(hgibbs_grm(dev, a0, a1 - a0, S.data(), ns.data()), "hgibbs_grm");
        double t = 0.0;
        hg_check(hgibbs_last_grm_ms(dev, &t), "hgibbs_last_grm_ms");
        ms += t;
        hg_check(hgibbs_grm_info(dev, &used, nullptr), "hgibbs_grm_info");
        size_t k = 0;
        for (unsigned a = a0; a < a1; ++a)
            for (unsigned b = 0; b <= a; ++b, ++k) {
                const double A = ns[k] ? S[k] / (double)ns[k] : std::numeric_limits<double>::quiet_NaN(); // the division in f64, one cast
                fa[k] = (float)A;
                fc[k] = (float)ns[k];
                if (fs && (a == b || A >= T)) {
                    std::fprintf(fs, "%u\t%u\t%.9g\n", a, b, A);
                    above += a != b;
                }
            }
        if (std::fwrite(fa.data(), sizeof(float), n, fb) != n) fatal("FATAL  : short write on " + binp);
        if (std::fwrite(fc.data(), sizeof(float), n, fn) != n) fatal("FATAL  : short write on " + nbinp);
        pairs += n;
        a0 = a1;
    }
    hgibbs_destroy(dev);
    close_out(fb, binp);
    close_out(fn, nbinp);
    if (fs) close_out(fs, spp);
    std::printf("GRM    : %u rows, %u of %u markers used, %llu entries written to %s (%.3f ms on the device)", N, used, co.Mtot, pairs, binp.c_str(), ms);
    if (fs) std::printf(", %llu off-diagonal pairs with A >= %g in %s", above, T, spp.c_str());
    std::printf("\n");
    return 0;
}

// The window of --ld-score, --clump and --ld-prune (`flag`) as an index interval per chromosome: every chromosome must be one run and,
// with a kb window, bp must not decrease inside it; ahead[j] = the markers of j's chromosome behind it within wsnps markers, resp.
// maxbp base pairs (two pointers), at most 4096 (the widest `op` takes)
struct LdWindow {
    std::vector<uint32_t> ahead;
    unsigned long long npairs = 0;
    uint32_t widest = 0;
    size_t nchroms = 0;
    std::string what; // the window in words, for the report: "<n> markers" or "<bp> bp"
};

LdWindow ld_window(const std::string& flag, const char* op, const BimRows& bim, const std::string& bimp, unsigned M, bool bySnps, long wsnps,
                   long long maxbp, const std::string& snpsOpt = "")
{
    const std::string bySnpsOpt = snpsOpt.empty() ? flag + "-snps" : snpsOpt; // the option that gives the window in markers
    auto marker = [&](unsigned j) { return bim.id[j] + " (row " + std::to_string(j + 1) + ")"; };
    std::map<std::string, int> chroms;
    for (unsigned j = 0; j < M; ++j) {
        if (j == 0 || bim.chr[j] != bim.chr[j - 1]) {
            if (!chroms.emplace(bim.chr[j], 1).second)
                fatal("FATAL  : " + bimp + ": chromosome " + bim.chr[j] + " comes back at marker " + marker(j) +
                      " after another chromosome: " + flag + " needs every chromosome as one contiguous run");
        } else if (!bySnps && bim.bp[j] < bim.bp[j - 1])
            fatal("FATAL  : " + bimp + ": bp decreases at marker " + marker(j) + " inside chromosome " + bim.chr[j] +
                  ": with a kb window the markers of a chromosome must be in bp order (the window must be an index interval; " + bySnpsOpt + " takes any order)");
    }
    LdWindow w;
    w.ahead.assign(M, 0);
    w.nchroms = chroms.size();
    w.what = bySnps ? std::to_string(wsnps) + " markers" : std::to_string(maxbp) + " bp";
    for (unsigned j = 0, e = 0; j < M; ++j) { // e: one past the last marker of j's window
        e = std::max(e, j + 1);
        while (e < M && bim.chr[e] == bim.chr[j] && (bySnps ? (long)(e - j) <= wsnps : bim.bp[e] - bim.bp[j] <= maxbp)) ++e;
        const unsigned n = e - 1 - j;
        if (n > 4096)
            fatal("FATAL  : marker " + marker(j) + " has " + std::to_string(n) + " markers ahead of it in its window, at most 4096 (the widest " + op + " takes): narrow the window");
        w.ahead[j] = n;
        w.npairs += n;
        w.widest = std::max(w.widest, n);
    }
    return w;
}

// ---- --ld-score: LD scores of the training markers on the chain's rows ----
int run_ldscore(const Options& opt, const Cohort& co)
{
    const std::string prefix = opt.ldScoreOut.empty() ? opt.mcmcOutDir + "/" + opt.mcmcOutNam : opt.ldScoreOut;
    const std::string bimp = opt.bedFile + ".bim";
    const unsigned M = co.Mtot;
    const BimRows bim = read_bim(bimp, M);

    // the window is an index interval per chromosome
    const bool bySnps = opt.ldScoreSnpsGiven;
    double kb = 1000.0;
    long wsnps = 0;
    if (opt.ldScoreKbGiven) whole_num(opt.ldScoreKb, kb);
    if (bySnps) whole_int(opt.ldScoreSnps, wsnps);
    const long long maxbp = (long long)std::llround(1000.0 * kb);
    const LdWindow win = ld_window("--ld-score", "hgibbs_ld_scores", bim, bimp, M, bySnps, wsnps, maxbp);
    const std::vector<uint32_t>& ahead = win.ahead;
    const unsigned long long npairs = win.npairs;
    const uint32_t widest = win.widest;
    const size_t nchroms = win.nchroms;
    const uint32_t W = std::max(1u, widest);

    // annotations: none (one column), or `base` and the sets or groups in definition order
    std::vector<std::string> colname;
    std::vector<uint64_t> annot;
    if (!opt.ldScoreSets.empty() || opt.ldScoreGroups) {
        const MarkerSets ms = opt.ldScoreSets.empty() ? sets_from_groups(opt, M) : read_sets_file(opt.ldScoreSets, opt.bedFile, bim, M);
        if (ms.idx.size() > 63)
            fatal("FATAL  : --ld-score: " + std::to_string(ms.idx.size()) + " annotations, at most 63 beside the base column (hgibbs_ld_scores takes 64 columns)");
        colname.push_back("base");
        annot.assign(M, 1ull);
        for (size_t c = 0; c < ms.idx.size(); ++c) {
            colname.push_back(ms.name[c]);
            for (const uint32_t j : ms.idx[c]) annot[j] |= 1ull << (c + 1);
        }
    }
    const uint32_t C = colname.empty() ? 1u : (uint32_t)colname.size();
    const std::string l2p = prefix + ".l2.ldscore", mp = prefix + ".l2.M", m5p = prefix + ".l2.M_5_50";
    std::printf("LDSCORE: %u markers, %zu chromosomes, window %s, %llu pairs in the window, widest window %u markers ahead, %u columns (%s r^2) -> %s\n", M,
                nchroms, win.what.c_str(), npairs, widest, C,
                opt.ldScoreRaw ? "raw" : "adjusted", l2p.c_str());
    std::fflush(stdout);
    if (!opt.ldScoreRaw && co.Ntot < 3) fatal("FATAL  : --ld-score: the adjusted r^2 - (1 - r^2) / (N - 2) needs at least three individuals (--ld-score-raw takes fewer)");

    std::vector<uint8_t> bed = read_training(opt.bedFile, co.numInds, M);
    if (opt.ldScoreOut.empty()) make_out_dir(opt);
    FILE* f = open_out(l2p, "w");
    FILE* fm = open_out(mp, "w");
    FILE* fm5 = open_out(m5p, "w");

    // the chain's rows and its standardisation; the counts give the allele frequencies
    hgibbs_t dev = open_training(co, bed);
    std::vector<double> mstd(M), l2((size_t)M * C);
    std::vector<uint64_t> n1(M), n2(M), nmiss(M);
    hg_check(hgibbs_marker_stats(dev, nullptr, mstd.data(), n1.data(), n2.data(), nmiss.data()), "hgibbs_marker_stats");
    hg_check(hgibbs_ld_scores(dev, W, ahead.data(), C, annot.empty() ? nullptr : annot.data(), opt.ldScoreRaw ? 0 : 1, l2.data()), "hgibbs_ld_scores");
    double products_ms = 0.0, reduce_ms = 0.0;
    hg_check(hgibbs_last_ld_scores_ms(dev, &products_ms, &reduce_ms), "hgibbs_last_ld_scores_ms");
    hgibbs_destroy(dev);

    std::fprintf(f, "CHR\tSNP\tBP");
    if (colname.empty()) std::fprintf(f, "\tL2");
    for (const std::string& n : colname) std::fprintf(f, "\t%sL2", n.c_str());
    std::fprintf(f, "\n");
    std::vector<unsigned long long> cnt(C, 0), cnt5(C, 0);
    unsigned written = 0;
    double sum0 = 0.0;
    for (unsigned j = 0; j < M; ++j) {
        if (!std::isfinite(mstd[j])) continue;
        const double called = (double)co.Ntot - (double)nmiss[j];
        const double p = called > 0.0 ? ((double)n1[j] + 2.0 * (double)n2[j]) / (2.0 * called) : 0.0;
        const bool common = std::min(p, 1.0 - p) > 0.05;
        std::fprintf(f, "%s\t%s\t%lld", bim.chr[j].c_str(), bim.id[j].c_str(), bim.bp[j]);
        for (uint32_t c = 0; c < C; ++c) {
            std::fprintf(f, "\t%.12g", l2[(size_t)j * C + c]);
            if (annot.empty() || ((annot[j] >> c) & 1ull)) {
                ++cnt[c];
                cnt5[c] += common ? 1u : 0u;
            }
        }
        std::fprintf(f, "\n");
        sum0 += l2[(size_t)j * C];
        ++written;
    }
    for (uint32_t c = 0; c < C; ++c) {
        std::fprintf(fm, "%s%llu", c ? "\t" : "", cnt[c]);
        std::fprintf(fm5, "%s%llu", c ? "\t" : "", cnt5[c]);
    }
    std::fprintf(fm, "\n");
    std::fprintf(fm5, "\n");
    close_out(f, l2p);
    close_out(fm, mp);
    close_out(fm5, m5p);
    std::printf("LDSCORE: wrote %u of %u markers to %s (%u without a finite sd left out), mean L2 of column 0 %.6g (products %.3f ms, reduce %.3f ms on the device)\n",
                written, M, l2p.c_str(), M - written, written ? sum0 / written : 0.0, products_ms, reduce_ms);
    return 0;
}

// ---- --clump, --ld-prune: LD clumping and pruning of the training markers ----
// the arguments of the two modes with their defaults (check_clump_args and check_ldprune_args have refused what does not parse)
double num_or(const std::string& t, double dflt)
{
    double v = dflt;
    if (!t.empty()) whole_num(t, v);
    return v;
}

// The table of --clump: the P of every row matched to the .bim by id (NaN: no usable row), and what was counted on the way
struct ClumpTable {
    std::vector<double> p; // per .bim marker
    unsigned rows = 0, matched = 0, unknown = 0, badp = 0;
};

ClumpTable read_clump_table(const std::string& path, const std::string& snpField, const std::string& pField, const BimRows& bim, unsigned M,
                            const std::string& bimp)
{
    std::ifstream in(path);
    if (!in) fatal("FATAL  : --clump: can not open the file [" + path + "] to read.");
    std::string line;
    if (!std::getline(in, line)) fatal("FATAL  : --clump: " + path + " has no header line");
    const std::vector<std::string> head = tokens(line, " \t\r");
    size_t cs = head.size(), cp = head.size();
    for (size_t c = 0; c < head.size(); ++c) {
        if (head[c] == snpField && cs == head.size()) cs = c;
        if (head[c] == pField && cp == head.size()) cp = c;
    }
    if (cs == head.size()) fatal("FATAL  : --clump: " + path + " has no column " + snpField + " in its header line (--clump-snp-field names the column of the marker ids)");
    if (cp == head.size()) fatal("FATAL  : --clump: " + path + " has no column " + pField + " in its header line (--clump-field names the column of the P values)");
    std::map<std::string, unsigned> at;
    for (unsigned j = 0; j < M; ++j)
        if (!at.emplace(bim.id[j], j).second) fatal("FATAL  : " + bimp + " lists SNP id " + bim.id[j] + " twice: --clump matches markers by id");
    ClumpTable t;
    t.p.assign(M, std::numeric_limits<double>::quiet_NaN());
    std::map<std::string, unsigned> seen; // id -> line
    for (unsigned ln = 2; std::getline(in, line); ++ln) {
        const std::vector<std::string> tok = tokens(line, " \t\r");
        if (tok.empty()) continue;
        if (tok.size() <= std::max(cs, cp))
            fatal("FATAL  : --clump: " + path + " line " + std::to_string(ln) + " has " + std::to_string(tok.size()) + " columns, the header names " + std::to_string(head.size()));
        ++t.rows;
        const auto first = seen.emplace(tok[cs], ln);
        if (!first.second)
            fatal("FATAL  : --clump: " + path + " line " + std::to_string(ln) + ": SNP id " + tok[cs] + " was already on line " + std::to_string(first.first->second) + ": one row per marker");
        const auto hit = at.find(tok[cs]);
        if (hit == at.end()) {
            ++t.unknown;
            continue;
        }
        ++t.matched;
        double v = 0.0;
        if (!whole_num(tok[cp], v) || !(v >= 0.0 && v <= 1.0)) { // NA, nan, anything that is no number in [0, 1]
            ++t.badp;
            continue;
        }
        t.p[hit->second] = v;
    }
    return t;
}

int run_ldselect(const Options& opt, const Cohort& co, bool clump)
{
    const std::string flag = clump ? "--clump" : "--ld-prune";
    const char* tag = clump ? "CLUMP  " : "PRUNE  ";
    const std::string base = opt.mcmcOutDir + "/" + opt.mcmcOutNam;
    const std::string bimp = opt.bedFile + ".bim";
    const unsigned M = co.Mtot;
    const BimRows bim = read_bim(bimp, M);

    // the window: kilobases (--clump: 250 unless markers are asked for) or markers (--ld-prune: 50 unless kilobases are asked for)
    const bool kbGiven = clump ? opt.clumpKbGiven : opt.ldPruneKbGiven, snpsGiven = clump ? opt.clumpSnpsGiven : opt.ldPruneSnpsGiven;
    const bool bySnps = clump ? snpsGiven : !kbGiven;
    const double kb = num_or(clump ? opt.clumpKb : opt.ldPruneKb, 250.0);
    long wsnps = 50;
    if (snpsGiven) whole_int(clump ? opt.clumpSnps : opt.ldPruneSnps, wsnps);
    const long long maxbp = (long long)std::llround(1000.0 * kb);
    const LdWindow win = ld_window(flag, "hgibbs_ld_mask", bim, bimp, M, bySnps, wsnps, maxbp);
    const uint32_t W = std::max(1u, win.widest);

    // who takes part, before the device knows which markers have a finite sd
    const double P1 = num_or(opt.clumpP1, 1e-4), P2 = num_or(opt.clumpP2, 1e-2), R2 = num_or(opt.clumpR2, 0.5), T = num_or(opt.ldPruneT, 0.0);
    ClumpTable tab;
    std::string out, outOut;
    if (clump) {
        tab = read_clump_table(opt.clumpFile, opt.clumpSnpField.empty() ? "SNP" : opt.clumpSnpField, opt.clumpField.empty() ? "P" : opt.clumpField, bim, M, bimp);
        out = opt.clumpOut.empty() ? base + ".clumped" : opt.clumpOut;
        unsigned part = 0, lead = 0;
        for (unsigned j = 0; j < M; ++j) {
            part += tab.p[j] <= P2 ? 1u : 0u;
            lead += tab.p[j] <= P1 ? 1u : 0u;
        }
        std::printf("%s: %u rows read from %s, %u matched to the .bim (%u ids not in it, %u without a P in [0, 1]), %u participating (P <= %g), %u able to lead (P <= %g), "
                    "window %s, %llu pairs in the window, widest window %u markers ahead, r^2 >= %g -> %s\n",
                    tag, tab.rows, opt.clumpFile.c_str(), tab.matched, tab.unknown, tab.badp, part, P2, lead, P1, win.what.c_str(), win.npairs, win.widest, R2, out.c_str());
    } else {
        const std::string prefix = opt.ldPruneOut.empty() ? base : opt.ldPruneOut;
        out = prefix + ".prune.in";
        outOut = prefix + ".prune.out";
        std::printf("%s: %u markers, %zu chromosomes, window %s, %llu pairs in the window, widest window %u markers ahead, r^2 > %g -> %s\n", tag, M, win.nchroms,
                    win.what.c_str(), win.npairs, win.widest, T, out.c_str());
    }
    std::fflush(stdout);

    std::vector<uint8_t> bed = read_training(opt.bedFile, co.numInds, M);
    if (clump ? opt.clumpOut.empty() : opt.ldPruneOut.empty()) make_out_dir(opt);
    FILE* f = open_out(out, "w");
    FILE* fo = clump ? nullptr : open_out(outOut, "w");

    // the chain's rows and its standardisation; the counts give the allele frequencies
    hgibbs_t dev = open_training(co, bed);
    std::vector<double> mstd(M);
    std::vector<uint64_t> n1(M), n2(M), nmiss(M);
    hg_check(hgibbs_marker_stats(dev, nullptr, mstd.data(), n1.data(), n2.data(), nmiss.data()), "hgibbs_marker_stats");

    // the order of priority: P ascending, resp. minor allele frequency descending; ties in .bim order
    std::vector<double> key(M, 0.0);
    std::vector<uint32_t> order;
    std::vector<uint8_t> mayLead;
    unsigned nosd = 0;
    if (clump) mayLead.assign(M, 0);
    for (unsigned j = 0; j < M; ++j) {
        if (clump) {
            if (!(tab.p[j] <= P2)) continue;
            if (!std::isfinite(mstd[j])) {
                ++nosd;
                continue;
            }
            key[j] = tab.p[j];
            mayLead[j] = tab.p[j] <= P1 ? 1 : 0;
        } else {
            if (!std::isfinite(mstd[j])) {
                ++nosd;
                continue;
            }
            const double called = (double)co.Ntot - (double)nmiss[j];
            const double p = called > 0.0 ? ((double)n1[j] + 2.0 * (double)n2[j]) / (2.0 * called) : 0.0;
            key[j] = -std::min(p, 1.0 - p);
        }
        order.push_back(j);
    }
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });

    // one bit per pair from the device, then the walk on the host
    const double t = clump ? R2 : std::nextafter(T, std::numeric_limits<double>::infinity());
    const size_t nm = (size_t)M * ((W + 63u) / 64u);
    std::vector<uint64_t> fwd(nm), bwd(nm);
    uint64_t npass = 0;
    hg_check(hgibbs_ld_mask(dev, W, win.ahead.data(), t, fwd.data(), bwd.data(), &npass), "hgibbs_ld_mask");
    double products_ms = 0.0, reduce_ms = 0.0;
    hg_check(hgibbs_last_ld_mask_ms(dev, &products_ms, &reduce_ms), "hgibbs_last_ld_mask_ms");
    hgibbs_destroy(dev);
    std::vector<int32_t> owner(M, -1);
    const double t0 = now_s();
    hg_check(hgibbs_ld_greedy(M, W, fwd.data(), bwd.data(), order.data(), (uint32_t)order.size(), clump ? mayLead.data() : nullptr, owner.data()), "hgibbs_ld_greedy");
    const double walk_ms = 1000.0 * (now_s() - t0);

    unsigned leaders = 0, claimed = 0;
    if (clump) {
        std::vector<std::vector<uint32_t>> members(M);
        for (unsigned j = 0; j < M; ++j)
            if (owner[j] >= 0 && (unsigned)owner[j] != j) members[owner[j]].push_back(j); // (.bim order)
        std::fprintf(f, "CHR F SNP BP P TOTAL NSIG S05 S01 S001 S0001 SP2\n");
        for (const uint32_t v : order) { // the leaders in the order they were taken
            if ((uint32_t)owner[v] != v) continue;
            unsigned bin[5] = {0, 0, 0, 0, 0};
            std::string sp2;
            for (const uint32_t q : members[v]) {
                const double pq = tab.p[q];
                ++bin[pq > 0.05 ? 0 : pq > 0.01 ? 1 : pq > 0.001 ? 2 : pq > 0.0001 ? 3 : 4];
                sp2 += (sp2.empty() ? "" : ",") + bim.id[q] + "(1)";
            }
            std::fprintf(f, "%s 1 %s %lld %.12g %zu %u %u %u %u %u %s\n", bim.chr[v].c_str(), bim.id[v].c_str(), bim.bp[v], tab.p[v], members[v].size(), bin[0],
                         bin[1], bin[2], bin[3], bin[4], sp2.empty() ? "NONE" : sp2.c_str());
            ++leaders;
            claimed += (unsigned)members[v].size();
        }
        close_out(f, out);
        std::printf("%s: %u clumps with %u markers claimed among %zu participating (%u without a finite sd left out), %llu passing pairs, wrote %s "
                    "(products %.3f ms, reduce %.3f ms on the device, the walk %.3f ms on the host)\n",
                    tag, leaders, claimed, order.size(), nosd, (unsigned long long)npass, out.c_str(), products_ms, reduce_ms, walk_ms);
    } else {
        for (unsigned j = 0; j < M; ++j) {
            const bool in = owner[j] >= 0 && (unsigned)owner[j] == j;
            std::fprintf(in ? f : fo, "%s\n", bim.id[j].c_str());
            leaders += in ? 1u : 0u;
        }
        close_out(f, out);
        close_out(fo, outOut);
        std::printf("%s: kept %u of %u markers in %s, %u in %s (%u without a finite sd among them), %llu passing pairs "
                    "(products %.3f ms, reduce %.3f ms on the device, the walk %.3f ms on the host)\n",
                    tag, leaders, M, out.c_str(), M - leaders, outOut.c_str(), nosd, (unsigned long long)npass, products_ms, reduce_ms, walk_ms);
    }
    return 0;
}

// ---- --he: Haseman-Elston regression on the chain's rows ----
int run_he(const Options& opt, const Cohort& co, const std::vector<double>& y_raw, const std::vector<double>& covX, int C)
{
    const std::string out = opt.heOut.empty() ? opt.mcmcOutDir + "/" + opt.mcmcOutNam + ".HEreg" : opt.heOut;
    const std::string rowsp = out + ".rows";
    const FamIds fam = read_fam_ids(opt.bedFile + ".fam", co.numInds, co.numNAs ? &co.keep : nullptr);
    const unsigned N = co.Ntot;
    if (fam.fid.size() != N) fatal("FATAL  : " + opt.bedFile + ".fam: " + std::to_string(fam.fid.size()) + " kept rows, expected " + std::to_string(N));
    if ((long long)N <= (long long)C + 2) fatal("FATAL  : --he needs more individuals (" + std::to_string(N) + ") than covariates + 2");

    // the chain's scaled phenotype; with covariates [1 | covariates] projected out as --assoc does, then scaled again
    std::vector<double> y(y_raw);
    scale_phenotype(y, N);
    if (C > 0) {
        CovProjector("--he", covX, C, N).project(y);
        scale_phenotype(y, N);
    }
    std::vector<uint8_t> bed = read_training(opt.bedFile, co.numInds, co.Mtot);
    if (opt.heOut.empty()) make_out_dir(opt);
    FILE* f = open_out(out, "w");
    FILE* fr = opt.heRows ? open_out(rowsp, "w") : nullptr;

    hgibbs_t dev = open_training(co, bed);
    std::vector<double> Y((size_t)2 * N), ay((size_t)2 * N), a1(N), a2(N), diag(N);
    std::vector<uint32_t> partners(N);
    for (unsigned i = 0; i < N; ++i) {
        Y[i] = y[i];
        Y[(size_t)N + i] = y[i] * y[i];
    }
    hg_check(hgibbs_grm_rowsums(dev, 2, Y.data(), ay.data(), a1.data(), a2.data(), diag.data(), partners.data()), "hgibbs_grm_rowsums");
    double products_ms = 0.0, reduce_ms = 0.0;
    hg_check(hgibbs_last_grm_rowsums_ms(dev, &products_ms, &reduce_ms), "hgibbs_last_grm_rowsums_ms");
    uint32_t used = 0;
    hg_check(hgibbs_grm_info(dev, &used, nullptr), "hgibbs_grm_info");
    hgibbs_destroy(dev);

    std::vector<double> ayv(N), ayy(N);
    for (unsigned i = 0; i < N; ++i) {
        ayv[i] = ay[(size_t)2 * i];
        ayy[i] = ay[(size_t)2 * i + 1];
    }
    for (unsigned i = 0; i < N; ++i)
        if (!partners[i])
            std::printf("WARNING: --he leaves out %s %s: it shares no called marker with anyone\n", fam.fid[i].c_str(), fam.iid[i].c_str());
    hgibbs_he_result res{};
    hg_check(hgibbs_he_fit(N, y.data(), ayv.data(), ayy.data(), a1.data(), a2.data(), partners.data(), &res), "hgibbs_he_fit");

    const hgibbs_he_form* forms[2] = {&res.cp, &res.sd};
    const char* names[2] = {"HE-CP", "HE-SD"};
    for (int k = 0; k < 2; ++k) {
        const hgibbs_he_form& r = *forms[k];
        std::fprintf(f, "%s%s\nCoefficient\tEstimate\tSE_OLS\tSE_Jackknife\tP_OLS\tP_Jackknife\n", k ? "\n" : "", names[k]);
        std::fprintf(f, "Intercept\t%.9g\t%.9g\t%.9g\t%.9g\t%.9g\n", r.intercept, r.intercept_se, r.intercept_se_jk, r.intercept_p, r.intercept_p_jk);
        std::fprintf(f, "V(G)/Vp\t%.9g\t%.9g\t%.9g\t%.9g\t%.9g\n", r.h2, r.h2_se, r.h2_se_jk, r.slope_p, r.slope_p_jk);
    }
    close_out(f, out);
    if (fr) {
        std::fprintf(fr, "FID\tIID\tNPARTNERS\tA_DIAG\tA_SUM\tA_SQSUM\tAY\n");
        for (unsigned i = 0; i < N; ++i)
            std::fprintf(fr, "%s\t%s\t%u\t%.12g\t%.12g\t%.12g\t%.12g\n", fam.fid[i].c_str(), fam.iid[i].c_str(), partners[i], diag[i], a1[i], a2[i], ayv[i]);
        close_out(fr, rowsp);
    }
    std::printf("HE     : %u rows, %u of %u markers used, %llu pairs, %u rows left out, %d covariates -> %s\n", N, used, co.Mtot,
                (unsigned long long)res.pairs, res.n_left_out, C, out.c_str());
    std::printf("HE     : HE-CP V(G)/Vp %.6g (SE %.3g OLS, %.3g jackknife), HE-SD V(G)/Vp %.6g (SE %.3g OLS, %.3g jackknife), Vp %.6g taken as fixed\n",
                res.cp.h2, res.cp.h2_se, res.cp.h2_se_jk, res.sd.h2, res.sd.h2_se, res.sd.h2_se_jk, res.vp);
    std::printf("HE     : products %.3f ms, reduce %.3f ms on the device", products_ms, reduce_ms);
    if (fr) std::printf(", the per-row sums in %s", rowsp.c_str());
    std::printf("\n");
    return 0;
}

// ---- --reml: REML heritability without the relationship matrix ----
struct RemlArgs {
    long trials = 15, cgIters = 200;
    double h2 = 0.25, cgTol = 1e-5, tol = 0.01;
};

// the values of --reml's options; refuses by name what is out of range
RemlArgs reml_args(const Options& opt)
{
    RemlArgs a;
    if (!opt.remlTrials.empty() && (!whole_int(opt.remlTrials, a.trials) || a.trials < 1 || a.trials > 31))
        fatal("FATAL  : --reml-trials " + opt.remlTrials + ": the number of probes must be an integer from 1 to 31 (with y, the 32 columns hgibbs_reml_solve takes)");
    if (!opt.remlH2.empty() && (!whole_num(opt.remlH2, a.h2) || !(a.h2 > 0.0 && a.h2 < 1.0)))
        fatal("FATAL  : --reml-h2-start " + opt.remlH2 + ": the start value must be a number inside (0, 1)");
    if (!opt.remlCgTol.empty() && (!whole_num(opt.remlCgTol, a.cgTol) || !std::isfinite(a.cgTol) || !(a.cgTol > 0.0)))
        fatal("FATAL  : --reml-cg-tol " + opt.remlCgTol + ": the tolerance must be a finite number > 0");
    if (!opt.remlCgIters.empty() && (!whole_int(opt.remlCgIters, a.cgIters) || a.cgIters < 1 || a.cgIters > std::numeric_limits<int>::max()))
        fatal("FATAL  : --reml-cg-iters " + opt.remlCgIters + ": needs at least one iteration");
    if (!opt.remlTol.empty() && (!whole_num(opt.remlTol, a.tol) || !std::isfinite(a.tol) || !(a.tol > 0.0)))
        fatal("FATAL  : --reml-tol " + opt.remlTol + ": the tolerance on log delta must be a finite number > 0");
    return a;
}

int run_reml(const Options& opt, const Cohort& co, const std::vector<double>& y_raw, const std::vector<double>& covX, int C)
{
    const RemlArgs args = reml_args(opt);
    const std::string out = opt.remlOut.empty() ? opt.mcmcOutDir + "/" + opt.mcmcOutNam + ".reml" : opt.remlOut;
    const std::string blupp = out + ".blup";
    const unsigned N = co.Ntot, M = co.Mtot;
    if (C > 31) fatal("FATAL  : --reml takes at most 31 covariates (" + std::to_string(C) + " given): with the column of ones, the 32 columns hgibbs_reml takes");
    if ((long long)N <= (long long)C + 2) fatal("FATAL  : --reml needs more individuals (" + std::to_string(N) + ") than covariates + 2");
    BimRows bim;
    if (opt.remlBlup) {
        bim = read_bim(opt.bedFile + ".bim", M);
        if (bim.id.size() != M) fatal("FATAL  : " + opt.bedFile + ".bim: " + std::to_string(bim.id.size()) + " rows, expected " + std::to_string(M));
    }

    // the phenotype of --he: the chain's scaling; with covariates [1 | covariates] projected out, then scaled again.  Z goes to the
    // library as well, whose P_c keeps every probe and iterate off its columns.
    std::vector<double> y(y_raw);
    scale_phenotype(y, N);
    const CovProjector proj("--reml", covX, C, N);
    if (C > 0) {
        proj.project(y);
        scale_phenotype(y, N);
    }
    std::vector<uint8_t> bed = read_training(opt.bedFile, co.numInds, M);
    if (opt.remlOut.empty()) make_out_dir(opt);
    FILE* f = open_out(out, "w");
    FILE* fb = opt.remlBlup ? open_out(blupp, "w") : nullptr;

    hgibbs_t dev = open_training(co, bed);
    hgibbs_reml_opts ro{};
    ro.trials = (int)args.trials;
    ro.h2_start = args.h2;
    ro.cg_tol = args.cgTol;
    ro.cg_iters = (int)args.cgIters;
    ro.x_tol = args.tol;
    ro.max_steps = 12;
    ro.seed = (uint64_t)opt.seed;
    hgibbs_reml_result r{};
    std::vector<double> blup(fb ? M : 0), mstd(fb ? M : 0), mave(fb ? M : 0);
    hg_check(hgibbs_reml(dev, &ro, proj.q, proj.Z.data(), y.data(), &r, fb ? blup.data() : nullptr), "hgibbs_reml");
    if (fb) {
        std::vector<uint64_t> n1(M), n2(M), nm(M);
        hg_check(hgibbs_marker_stats(dev, mave.data(), mstd.data(), n1.data(), n2.data(), nm.data()), "hgibbs_marker_stats");
    }
    hgibbs_destroy(dev);

    const hgibbs_reml_estimate& e = r.est;
    const char* status = r.status == HGIBBS_REML_AT_BOUND ? "AT_BOUND" : "CONVERGED";
    int cg = 0;
    for (int k = 0; k < r.steps; ++k) cg += r.cg_iters[k];
    std::fprintf(f, "Source\tVariance\tSE\n");
    std::fprintf(f, "V(G)\t%.9g\t%.9g\nV(e)\t%.9g\t%.9g\nVp\t%.9g\t%.9g\nV(G)/Vp\t%.9g\t%.9g\n", e.vg, e.se_vg, e.ve, e.se_ve, e.vp, e.se_vp, e.h2, e.se_h2);
    std::fprintf(f, "logdelta\t%.9g\nSE_MC\t%.9g\nn\t%u\nM_used\t%u\nq\t%d\ntrials\t%d\nsteps\t%d\ncg_iters\t%d\nstatus\t%s\n", e.logdelta, e.se_mc, r.n, r.m_used,
                 r.q, r.trials, r.steps, cg, status);
    close_out(f, out);
    if (fb) {
        std::fprintf(fb, "CHR\tSNP\tBP\tA1\tA2\tBETA\n");
        for (unsigned j = 0; j < M; ++j) {
            std::fprintf(fb, "%s\t%s\t%lld\t%s\t%s\t", bim.chr[j].c_str(), bim.id[j].c_str(), bim.bp[j], bim.a1[j].c_str(), bim.a2[j].c_str());
            if (std::isfinite(mstd[j])) std::fprintf(fb, "%.9g\n", blup[j] * mstd[j]);
            else std::fprintf(fb, "NA\n");
        }
        close_out(fb, blupp);
    }
    if (r.status == HGIBBS_REML_AT_BOUND) std::printf("WARNING: --reml stopped at the bound of its search, |log delta| = log 9999: the estimate is the bound, not a root\n");
    std::printf("REML   : %u rows, %u of %u markers used, %d covariates, %d probes (seed %u), %d evaluations, %d CG iterations, %s -> %s\n", N, r.m_used, M, C, r.trials,
                opt.seed, r.steps, cg, status, out.c_str());
    std::printf("REML   : V(G)/Vp %.6g (SE %.3g, SE_MC %.3g), V(G) %.6g, V(e) %.6g, log delta %.6g; products %.3f ms, algebra %.3f ms on the device", e.h2, e.se_h2,
                e.se_mc, e.vg, e.ve, e.logdelta, r.products_ms, r.algebra_ms);
    if (fb) std::printf(", the marker effects in %s", blupp.c_str());
    std::printf("\n");
    return 0;
}

// ---- --qc: quality control of the chain's rows and the training markers ----
// a number as the tables print it: nine digits, NA when it is not defined
std::string qc_num(double v)
{
    if (!std::isfinite(v)) return "NA";
    char b[32];
    std::snprintf(b, sizeof b, "%.9g", v);
    return b;
}

int run_qc(const Options& opt, const Cohort& co)
{
    const std::string prefix = opt.qcOut.empty() ? opt.mcmcOutDir + "/" + opt.mcmcOutNam : opt.qcOut;
    const bool markerT = opt.qcMafGiven || opt.qcGenoGiven || opt.qcHweGiven, rowT = opt.qcMindGiven || opt.qcHetSdGiven;
    double tMaf = 0.0, tGeno = 0.0, tMind = 0.0, tHwe = 0.0, tHet = 0.0;
    whole_num(opt.qcMaf, tMaf);
    whole_num(opt.qcGeno, tGeno);
    whole_num(opt.qcMind, tMind);
    whole_num(opt.qcHwe, tHwe);
    whole_num(opt.qcHetSd, tHet);
    const FamIds fam = read_fam_ids(opt.bedFile + ".fam", co.numInds, co.numNAs ? &co.keep : nullptr);
    const unsigned N = co.Ntot, M = co.Mtot;
    if (fam.fid.size() != N) fatal("FATAL  : " + opt.bedFile + ".fam: " + std::to_string(fam.fid.size()) + " kept rows, expected " + std::to_string(N));
    const BimRows bim = read_bim(opt.bedFile + ".bim", M);
    if (bim.id.size() != M) fatal("FATAL  : " + opt.bedFile + ".bim: " + std::to_string(bim.id.size()) + " rows, expected " + std::to_string(M));
    std::vector<uint8_t> bed = read_training(opt.bedFile, co.numInds, M);
    if (opt.qcOut.empty()) make_out_dir(opt);
    const char* const ext[6] = {".frq", ".lmiss", ".hwe", ".imiss", ".het", ".ibc"};
    const char* const head[6] = {"CHR\tSNP\tA1\tA2\tMAF\tNCHROBS\n",        "CHR\tSNP\tN_MISS\tN_GENO\tF_MISS\n", "CHR\tSNP\tTEST\tA1\tA2\tGENO\tO(HET)\tE(HET)\tP\n",
                                 "FID\tIID\tN_MISS\tN_GENO\tF_MISS\n",      "FID\tIID\tO(HOM)\tE(HOM)\tN(NM)\tF\n", "FID\tIID\tNOMISS\tFhat1\tFhat2\tFhat3\n"};
    FILE* f[6];
    for (int k = 0; k < 6; ++k) {
        f[k] = open_out(prefix + ext[k], "w");
        std::fputs(head[k], f[k]);
    }
    FILE* fx = markerT ? open_out(prefix + ".qc.exclude", "w") : nullptr;
    FILE* fr = rowT ? open_out(prefix + ".qc.remove", "w") : nullptr;
    if (fx) std::fputs("SNP\tREASON\n", fx);
    if (fr) std::fputs("FID\tIID\tREASON\n", fr);

    hgibbs_t dev = open_training(co, bed);
    std::vector<double> mave(M), mstd(M);
    std::vector<uint64_t> n1(M), n2(M), nm(M);
    hg_check(hgibbs_marker_stats(dev, mave.data(), mstd.data(), n1.data(), n2.data(), nm.data()), "hgibbs_marker_stats");

    // the seven tables: t0 missing calls over every marker; over the QC markers (a finite sd, chromosome 1 .. 22)
    // t1 called, t2 homozygous, t3 expected homozygosity, t4 .. t6 the terms of GCTA's Fhat1 .. Fhat3
    const int T = 7;
    std::vector<double> tab((size_t)T * M * 4, 0.0);
    std::vector<uint8_t> qcm(M, 0);
    unsigned nqc = 0;
    for (unsigned j = 0; j < M; ++j) {
        auto at = [&](int t) { return &tab[((size_t)t * M + j) * 4]; };
        at(0)[3] = 1.0;
        long chr = 0;
        if (!std::isfinite(mstd[j]) || !whole_int(bim.chr[j], chr) || chr < 1 || chr > 22) continue;
        qcm[j] = 1;
        ++nqc;
        const double nc = (double)(N - nm[j]), p = ((double)n1[j] + 2.0 * (double)n2[j]) / (2.0 * nc), h = 2.0 * p * (1.0 - p);
        const double e = 1.0 - h * (2.0 * nc) / (2.0 * nc - 1.0);
        for (int g = 0; g < 3; ++g) {
            const double x = (double)g;
            at(1)[g] = 1.0;
            at(2)[g] = g == 1 ? 0.0 : 1.0;
            at(3)[g] = e;
            at(4)[g] = (x - 2.0 * p) * (x - 2.0 * p) / h - 1.0;
            at(5)[g] = 1.0 - x * (2.0 - x) / h;
            at(6)[g] = (x * x - (1.0 + 2.0 * p) * x + 2.0 * p * p) / h;
        }
    }
    std::vector<double> sums((size_t)N * T);
    hg_check(hgibbs_row_sums(dev, T, tab.data(), sums.data()), "hgibbs_row_sums");
    double ms = 0.0;
    hg_check(hgibbs_last_row_sums_ms(dev, &ms), "hgibbs_last_row_sums_ms");
    hgibbs_destroy(dev);

    // per marker, in .bim order
    const double NaN = std::numeric_limits<double>::quiet_NaN();
    unsigned xMono = 0, xMaf = 0, xGeno = 0, xHwe = 0, xAny = 0;
    for (unsigned j = 0; j < M; ++j) {
        const uint64_t ncl = (uint64_t)N - nm[j], n0 = ncl - n1[j] - n2[j];
        const double p = ncl ? ((double)n1[j] + 2.0 * (double)n2[j]) / (2.0 * (double)ncl) : NaN;
        const double fmiss = (double)nm[j] / (double)N;
        double P = NaN;
        hg_check(hgibbs_hwe_exact((uint32_t)n1[j], (uint32_t)n2[j], (uint32_t)n0, &P), "hgibbs_hwe_exact");
        const char *chr = bim.chr[j].c_str(), *id = bim.id[j].c_str(), *a1 = bim.a1[j].c_str(), *a2 = bim.a2[j].c_str();
        std::fprintf(f[0], "%s\t%s\t%s\t%s\t%s\t%llu\n", chr, id, a1, a2, qc_num(p).c_str(), 2ull * ncl);
        std::fprintf(f[1], "%s\t%s\t%llu\t%u\t%s\n", chr, id, (unsigned long long)nm[j], N, qc_num(fmiss).c_str());
        std::fprintf(f[2], "%s\t%s\tALL\t%s\t%s\t%llu/%llu/%llu\t%s\t%s\t%s\n", chr, id, a1, a2, (unsigned long long)n2[j], (unsigned long long)n1[j],
                     (unsigned long long)n0, qc_num(ncl ? (double)n1[j] / (double)ncl : NaN).c_str(), qc_num(2.0 * p * (1.0 - p)).c_str(), qc_num(P).c_str());
        if (!fx) continue;
        std::string why;
        auto add = [&](const char* r) { why += (why.empty() ? "" : ","); why += r; };
        if (!std::isfinite(mstd[j])) {
            add("MONO");
            ++xMono;
        } else {
            if (opt.qcMafGiven && std::min(p, 1.0 - p) < tMaf) add("MAF"), ++xMaf;
            if (opt.qcGenoGiven && fmiss > tGeno) add("GENO"), ++xGeno;
            if (opt.qcHweGiven && P < tHwe) add("HWE"), ++xHwe;
        }
        if (!why.empty()) {
            std::fprintf(fx, "%s\t%s\n", id, why.c_str());
            ++xAny;
        }
    }

    // per kept row, in .fam order
    std::vector<double> F(N, NaN);
    for (unsigned i = 0; i < N; ++i) {
        const double* s = &sums[(size_t)i * T];
        if (s[1] > 0.0 && s[1] - s[3] != 0.0) F[i] = (s[2] - s[3]) / (s[1] - s[3]);
    }
    double fmean = NaN, fsd = NaN;
    {
        long double a = 0.0L, q = 0.0L;
        unsigned k = 0;
        for (unsigned i = 0; i < N; ++i)
            if (std::isfinite(F[i])) a += F[i], ++k;
        if (k >= 2) {
            a /= k;
            for (unsigned i = 0; i < N; ++i)
                if (std::isfinite(F[i])) q += ((long double)F[i] - a) * ((long double)F[i] - a);
            fmean = (double)a;
            fsd = (double)std::sqrt(q / (k - 1));
        }
    }
    unsigned rMind = 0, rHet = 0, rAny = 0;
    for (unsigned i = 0; i < N; ++i) {
        const double* s = &sums[(size_t)i * T];
        const char *fid = fam.fid[i].c_str(), *iid = fam.iid[i].c_str();
        const double fmiss = s[0] / (double)M, nn = s[1];
        std::fprintf(f[3], "%s\t%s\t%.0f\t%u\t%s\n", fid, iid, s[0], M, qc_num(fmiss).c_str());
        std::fprintf(f[4], "%s\t%s\t%.0f\t%s\t%.0f\t%s\n", fid, iid, s[2], qc_num(s[3]).c_str(), nn, qc_num(F[i]).c_str());
        std::fprintf(f[5], "%s\t%s\t%.0f\t%s\t%s\t%s\n", fid, iid, nn, qc_num(nn > 0.0 ? s[4] / nn : NaN).c_str(), qc_num(nn > 0.0 ? s[5] / nn : NaN).c_str(),
                     qc_num(nn > 0.0 ? s[6] / nn : NaN).c_str());
        if (!fr) continue;
        std::string why;
        if (opt.qcMindGiven && fmiss > tMind) why = "MIND", ++rMind;
        if (opt.qcHetSdGiven && std::isfinite(F[i]) && std::isfinite(fsd) && std::fabs(F[i] - fmean) > tHet * fsd) why += (why.empty() ? "HET" : ",HET"), ++rHet;
        if (!why.empty()) {
            std::fprintf(fr, "%s\t%s\t%s\n", fid, iid, why.c_str());
            ++rAny;
        }
    }
    for (int k = 0; k < 6; ++k) close_out(f[k], prefix + ext[k]);
    if (fx) close_out(fx, prefix + ".qc.exclude");
    if (fr) close_out(fr, prefix + ".qc.remove");
    std::printf("QC     : %u rows, %u markers (%u enter the per-row statistics) -> %s.{frq,lmiss,hwe,imiss,het,ibc} (row sums %.3f ms on the device)\n", N, M, nqc,
                prefix.c_str(), ms);
    std::printf("QC     : markers listed %u (MONO %u, MAF %u, GENO %u, HWE %u)%s; rows listed %u (MIND %u, HET %u)%s\n", xAny, xMono, xMaf, xGeno, xHwe,
                fx ? "" : " [no marker threshold]", rAny, rMind, rHet, fr ? "" : " [no row threshold]");
    return 0;
}

// ---- --homozyg: runs of homozygosity of the chain's rows ----
// PLINK 1.9's defaults; an argument that was given is parsed as a whole and refused by name when it is out of range (check_homozyg_args
// calls this before anything is read, run_homozyg again for the values)
struct HomozygArgs {
    long window = 50, windowHet = 1, windowMissing = 5, snp = 100, het = -1; // het: -1 = no limit
    double threshold = 0.05, kb = 1000.0, density = 50.0, gap = 1000.0;
};

HomozygArgs homozyg_args(const Options& opt)
{
    HomozygArgs a;
    auto count = [](const char* flag, const std::string& t, long lo, long hi, const char* what, long& v) {
        long x = 0;
        if (t.empty()) return;
        if (!whole_int(t, x) || x < lo || x > hi) fatal(std::string("FATAL  : ") + flag + " " + t + ": " + what);
        v = x;
    };
    auto kilobases = [](const char* flag, const std::string& t, const char* what, double& v) {
        double x = 0.0;
        if (t.empty()) return;
        if (!whole_num(t, x) || !std::isfinite(x) || x < 0.0 || x > 1e12) fatal(std::string("FATAL  : ") + flag + " " + t + ": " + what);
        v = x;
    };
    count("--homozyg-window-snp", opt.hzWindow, 1, 64, "the window must be an integer from 1 to 64 markers (the widest hgibbs_roh takes: a window is one 64-bit word)", a.window);
    count("--homozyg-window-het", opt.hzWindowHet, 0, 64, "the hets a window may hold must be an integer from 0 to 64", a.windowHet);
    count("--homozyg-window-missing", opt.hzWindowMissing, 0, 64, "the missing calls a window may hold must be an integer from 0 to 64", a.windowMissing);
    count("--homozyg-snp", opt.hzSnp, 1, 2147483647, "the markers a segment needs must be an integer >= 1", a.snp);
    count("--homozyg-het", opt.hzHet, 0, 2147483647, "the hets a segment may hold must be an integer >= 0", a.het);
    if (!opt.hzThreshold.empty() && (!whole_num(opt.hzThreshold, a.threshold) || !(a.threshold > 0.0 && a.threshold <= 1.0)))
        fatal("FATAL  : --homozyg-window-threshold " + opt.hzThreshold + ": the share of homozygous windows must be a number in (0, 1]");
    kilobases("--homozyg-kb", opt.hzKb, "the length a segment needs must be a finite number of kilobases from 0 to 1e12", a.kb);
    kilobases("--homozyg-density", opt.hzDensity, "the kilobases per marker a segment may have must be a finite number from 0 to 1e12", a.density);
    kilobases("--homozyg-gap", opt.hzGap, "the gap that cuts a segment must be a finite number of kilobases from 0 to 1e12", a.gap);
    return a;
}

int run_homozyg(const Options& opt, const Cohort& co)
{
    const std::string prefix = opt.hzOut.empty() ? opt.mcmcOutDir + "/" + opt.mcmcOutNam : opt.hzOut;
    const std::string bimp = opt.bedFile + ".bim";
    const HomozygArgs ha = homozyg_args(opt);
    hgibbs_roh_params p{};
    p.window = (uint32_t)ha.window;
    p.window_het = (uint32_t)ha.windowHet;
    p.window_missing = (uint32_t)ha.windowMissing;
    for (uint32_t n = 1; n <= p.window; ++n) { // the smallest c with c / n >= threshold: the device compares integers only
        uint32_t c = 1;
        while ((double)c / (double)n < ha.threshold) ++c;
        p.need[n] = c;
    }
    p.min_snps = (uint32_t)ha.snp;
    p.min_bp = (int64_t)std::llround(ha.kb * 1000.0);
    p.dens_bp = (int64_t)std::llround(ha.density * 1000.0);
    p.gap_bp = (int64_t)std::llround(ha.gap * 1000.0);
    p.max_het = ha.het < 0 ? UINT32_MAX : (uint32_t)ha.het;

    const FamIds fam = read_fam_ids(opt.bedFile + ".fam", co.numInds, co.numNAs ? &co.keep : nullptr);
    const unsigned N = co.Ntot, M = co.Mtot;
    if (fam.fid.size() != N) fatal("FATAL  : " + opt.bedFile + ".fam: " + std::to_string(fam.fid.size()) + " kept rows, expected " + std::to_string(N));
    const BimRows bim = read_bim(bimp, M);
    if (bim.id.size() != M) fatal("FATAL  : " + bimp + ": " + std::to_string(bim.id.size()) + " rows, expected " + std::to_string(M));
    // an autosome (chromosome 1 .. 22) must be one run of the .bim, in bp order: a segment is an index interval
    const ChromRuns cr(bim, M);
    std::vector<uint8_t> autosome(cr.nruns, 0);
    {
        auto marker = [&](unsigned j) { return bim.id[j] + " (row " + std::to_string(j + 1) + ")"; };
        std::vector<uint8_t> seen(cr.nchrom, 0);
        for (size_t r = 0; r < cr.nruns; ++r) {
            const unsigned j0 = cr.runs[r], j1 = cr.runs[r + 1];
            long chr = 0;
            if (!whole_int(bim.chr[j0], chr) || chr < 1 || chr > 22) continue;
            autosome[r] = 1;
            if (seen[cr.cj[j0]])
                fatal("FATAL  : " + bimp + ": chromosome " + bim.chr[j0] + " comes back at marker " + marker(j0) +
                      " after another chromosome: --homozyg needs every chromosome as one contiguous run");
            seen[cr.cj[j0]] = 1;
            for (unsigned j = j0; j < j1; ++j) {
                if (j > j0 && bim.bp[j] < bim.bp[j - 1])
                    fatal("FATAL  : " + bimp + ": bp decreases at marker " + marker(j) + " inside chromosome " + bim.chr[j] +
                          ": --homozyg needs the markers of a chromosome in bp order (a segment must be an index interval)");
                if (bim.bp[j] < 0) fatal("FATAL  : " + bimp + ": marker " + marker(j) + " has a negative bp");
            }
        }
    }
    std::vector<uint8_t> bed = read_training(opt.bedFile, co.numInds, M);
    if (opt.hzOut.empty()) make_out_dir(opt);
    FILE* fh = open_out(prefix + ".hom", "w");
    FILE* fi = open_out(prefix + ".hom.indiv", "w");
    FILE* fs = open_out(prefix + ".hom.summary", "w");
    std::fputs("FID\tIID\tCHR\tSNP1\tSNP2\tPOS1\tPOS2\tKB\tNSNP\tDENSITY\tPHOM\tPHET\n", fh);
    std::fputs("FID\tIID\tNSEG\tKB\tKBAVG\tFROH\n", fi);
    std::fputs("CHR\tSNP\tBP\tN_ROH\n", fs);

    hgibbs_t dev = open_training(co, bed);
    std::vector<double> mstd(M);
    hg_check(hgibbs_marker_stats(dev, nullptr, mstd.data(), nullptr, nullptr, nullptr), "hgibbs_marker_stats");
    // the selection: --qc's QC markers (a finite sd, chromosome 1 .. 22), one run per chromosome
    std::vector<uint32_t> run_off{0}, idx;
    std::vector<int64_t> bp;
    long long span = 0; // sum over chromosomes of last selected bp - first selected bp
    for (size_t r = 0; r < cr.nruns; ++r) {
        if (!autosome[r]) continue;
        for (unsigned j = cr.runs[r]; j < cr.runs[r + 1]; ++j)
            if (std::isfinite(mstd[j])) idx.push_back(j), bp.push_back(bim.bp[j]);
        if (idx.size() == run_off.back()) continue; // nothing selected on this chromosome
        span += bp.back() - bp[run_off.back()];
        run_off.push_back((uint32_t)idx.size());
    }
    const uint32_t nruns = (uint32_t)run_off.size() - 1u;
    uint64_t nseg = 0;
    hg_check(hgibbs_roh(dev, nruns, run_off.data(), idx.data(), bp.data(), &p, &nseg), "hgibbs_roh");
    std::vector<hgibbs_roh_seg> segs(nseg);
    hg_check(hgibbs_roh_get(dev, segs.data()), "hgibbs_roh_get");
    double ms = 0.0;
    hg_check(hgibbs_last_roh_ms(dev, &ms), "hgibbs_last_roh_ms");
    hgibbs_destroy(dev);

    // the list is sorted by (row, first): rows in .fam order, then by position
    std::vector<long long> diff(idx.size() + 1, 0); // per position: rows whose segment starts here minus rows whose segment ended before
    unsigned rowsWith = 0;
    size_t s = 0;
    for (unsigned i = 0; i < N; ++i) {
        unsigned k = 0;
        long long sum = 0;
        for (; s < segs.size() && segs[s].row == i; ++s, ++k) {
            const hgibbs_roh_seg& g = segs[s];
            const unsigned j1 = idx[g.first], j2 = idx[g.last];
            const long long len = bp[g.last] - bp[g.first];
            const double kb = (double)len / 1000.0, n = (double)g.nsnp;
            sum += len;
            diff[g.first] += 1;
            diff[g.last + 1] -= 1;
            std::fprintf(fh, "%s\t%s\t%s\t%s\t%s\t%lld\t%lld\t%s\t%u\t%s\t%s\t%s\n", fam.fid[i].c_str(), fam.iid[i].c_str(), bim.chr[j1].c_str(), bim.id[j1].c_str(),
                         bim.id[j2].c_str(), (long long)bp[g.first], (long long)bp[g.last], qc_num(kb).c_str(), g.nsnp, qc_num(kb / n).c_str(),
                         qc_num((double)(g.nsnp - g.nhet - g.nmiss) / n).c_str(), qc_num((double)g.nhet / n).c_str());
        }
        if (k) ++rowsWith;
        const double kb = (double)sum / 1000.0;
        std::fprintf(fi, "%s\t%s\t%u\t%s\t%s\t%s\n", fam.fid[i].c_str(), fam.iid[i].c_str(), k, qc_num(kb).c_str(), k ? qc_num(kb / (double)k).c_str() : "NA",
                     span > 0 ? qc_num((double)sum / (double)span).c_str() : "NA");
    }
    // per .bim marker: the rows with a segment over it (a segment lies inside one run, so one running sum serves every chromosome)
    {
        size_t k = 0;
        long long over = 0;
        for (unsigned j = 0; j < M; ++j) {
            if (k < idx.size() && idx[k] == j) {
                over += diff[k++];
                std::fprintf(fs, "%s\t%s\t%lld\t%lld\n", bim.chr[j].c_str(), bim.id[j].c_str(), bim.bp[j], over);
            } else
                std::fprintf(fs, "%s\t%s\t%lld\tNA\n", bim.chr[j].c_str(), bim.id[j].c_str(), bim.bp[j]);
        }
    }
    close_out(fh, prefix + ".hom");
    close_out(fi, prefix + ".hom.indiv");
    close_out(fs, prefix + ".hom.summary");
    std::printf("HOMOZYG: %u rows, %zu of %u markers selected on %u chromosomes; window %ld markers (%ld het, %ld missing, threshold %g), segments of >= %ld markers, >= %g kb, "
                "<= %g kb per marker, gap %g kb%s\n",
                N, idx.size(), M, nruns, ha.window, ha.windowHet, ha.windowMissing, ha.threshold, ha.snp, ha.kb, ha.density, ha.gap,
                ha.het < 0 ? "" : (", <= " + std::to_string(ha.het) + " hets").c_str());
    std::printf("HOMOZYG: %llu segments in %u rows -> %s.{hom,hom.indiv,hom.summary} (%.3f ms on the device)\n", (unsigned long long)nseg, rowsWith, prefix.c_str(), ms);
    return 0;
}

// ---- --epistasis: BOOST's pairwise interaction scan of a case/control phenotype ----
struct EpistasisArgs {
    double chisq = 30.0, gapKb = -1.0; // BOOST's screening threshold; gapKb < 0: no gap
};

EpistasisArgs epistasis_args(const Options& opt)
{
    EpistasisArgs a;
    if (!opt.epiChisq.empty() && (!whole_num(opt.epiChisq, a.chisq) || !std::isfinite(a.chisq) || !(a.chisq > 0.0)))
        fatal("FATAL  : --epistasis-chisq " + opt.epiChisq + ": the threshold on the statistic must be a finite number > 0");
    if (!opt.epiGap.empty() && (!whole_num(opt.epiGap, a.gapKb) || !std::isfinite(a.gapKb) || a.gapKb < 0.0 || a.gapKb > 1e12))
        fatal("FATAL  : --epistasis-gap " + opt.epiGap + ": the gap must be a finite number of kilobases from 0 to 1e12");
    return a;
}

int run_epistasis(const Options& opt, const Cohort& co, const std::vector<double>& y_raw)
{
    const std::string out = opt.epiOut.empty() ? opt.mcmcOutDir + "/" + opt.mcmcOutNam + ".epi.cc" : opt.epiOut;
    const EpistasisArgs ea = epistasis_args(opt);
    const unsigned N = co.Ntot, M = co.Mtot;
    const std::vector<double> vals = case_control_values("--epistasis", y_raw, N);
    std::vector<uint8_t> cls(N);
    unsigned ncase = 0;
    for (unsigned i = 0; i < N; ++i) ncase += cls[i] = y_raw[i] == vals[1] ? 1 : 0;
    const BimRows bim = read_bim(opt.bedFile + ".bim", M);
    if (bim.id.size() != M) fatal("FATAL  : " + opt.bedFile + ".bim: " + std::to_string(bim.id.size()) + " rows, expected " + std::to_string(M));
    // the lists: every marker against every later one, or the one or two sets of --epistasis-sets
    std::vector<uint32_t> listA, listB;
    bool two = false;
    size_t unknown = 0;
    if (opt.epiSets.empty()) {
        listA.resize(M);
        for (unsigned j = 0; j < M; ++j) listA[j] = j;
    } else {
        const MarkerSets ms = read_sets_file(opt.epiSets, opt.bedFile, bim, M, &unknown);
        if (ms.idx.size() > 2)
            fatal("FATAL  : --epistasis-sets " + opt.epiSets + " names " + std::to_string(ms.idx.size()) + " sets (" + ms.name[0] + ", " + ms.name[1] + ", " + ms.name[2] +
                  (ms.idx.size() > 3 ? ", ..." : "") + "): one set is scanned within itself, two against each other, more are not taken");
        for (size_t s = 0; s < ms.idx.size(); ++s)
            if (ms.idx[s].empty()) fatal("FATAL  : --epistasis-sets " + opt.epiSets + ": set " + ms.name[s] + " is empty (none of its ids is in " + opt.bedFile + ".bim)");
        listA = ms.idx[0];
        two = ms.idx.size() == 2;
        if (two) listB = ms.idx[1];
    }
    auto count_pairs = [&](const std::vector<uint32_t>& A, const std::vector<uint32_t>& B) {
        if (!two) return (unsigned long long)A.size() * (A.size() - (A.empty() ? 0 : 1)) / 2ull;
        std::vector<uint8_t> inA(M, 0);
        for (const uint32_t j : A) inA[j] = 1;
        unsigned long long both = 0;
        for (const uint32_t j : B) both += inA[j];
        return (unsigned long long)A.size() * B.size() - both - both * (both - (both ? 1 : 0)) / 2ull; // less (x, x), and (x, y) with (y, x) once
    };
    std::printf("EPISTASIS: %u rows (%u cases, %u controls); %zu markers%s listed, %llu pairs; CHISQ >= %g%s%s\n", N, ncase, N - ncase, listA.size() + listB.size(),
                two ? " in two sets" : "", count_pairs(listA, listB), ea.chisq, ea.gapKb < 0.0 ? "" : (", gap " + qc_num(ea.gapKb) + " kb").c_str(),
                unknown ? (", " + std::to_string(unknown) + " ids of the sets are not in the .bim").c_str() : "");
    std::vector<uint8_t> bed = read_training(opt.bedFile, co.numInds, M);
    if (opt.epiOut.empty()) make_out_dir(opt);
    FILE* f = open_out(out, "w");
    std::fputs("CHR1\tSNP1\tBP1\tCHR2\tSNP2\tBP2\tN\tN_CASE\tN_CTRL\tKSA\tCHISQ\tDF\tP\tOK\n", f);

    hgibbs_t dev = open_training(co, bed);
    std::vector<double> mstd(M);
    hg_check(hgibbs_marker_stats(dev, nullptr, mstd.data(), nullptr, nullptr, nullptr), "hgibbs_marker_stats");
    // a marker without a finite sd (monomorphic, or never called) has one category at most: no interaction to test
    size_t dropped = 0;
    for (std::vector<uint32_t>* l : {&listA, &listB}) {
        const size_t before = l->size();
        l->erase(std::remove_if(l->begin(), l->end(), [&](uint32_t j) { return !std::isfinite(mstd[j]); }), l->end());
        dropped += before - l->size();
    }
    const unsigned long long tested = count_pairs(listA, listB);
    uint64_t nlist = 0;
    double pms = 0.0, sms = 0.0;
    std::vector<uint32_t> ab;
    std::vector<int32_t> tab;
    if (!listA.empty() && (!two || !listB.empty()) && tested) {
        hg_check(hgibbs_epi_scan(dev, (uint32_t)listA.size(), listA.data(), (uint32_t)listB.size(), two ? listB.data() : nullptr, cls.data(), ea.chisq, &nlist), "hgibbs_epi_scan");
        ab.resize(2 * nlist);
        tab.resize(18 * nlist);
        hg_check(hgibbs_epi_scan_get(dev, ab.data(), tab.data(), nullptr), "hgibbs_epi_scan_get");
        hg_check(hgibbs_last_epi_ms(dev, &pms, &sms), "hgibbs_last_epi_ms");
    }
    hgibbs_destroy(dev);

    // the listed pairs as (first, second) in .bim order with the table turned to match; a pair of two sets that was reached in both
    // orders is kept once, a marker against itself never
    struct Row {
        uint32_t j1, j2;
        int32_t t[18];
    };
    std::vector<Row> rows;
    rows.reserve(nlist);
    for (uint64_t p = 0; p < nlist; ++p) {
        const uint32_t ja = listA[ab[2 * p]], jb = (two ? listB : listA)[ab[2 * p + 1]];
        if (ja == jb) continue;
        Row r;
        r.j1 = std::min(ja, jb);
        r.j2 = std::max(ja, jb);
        for (int k = 0; k < 2; ++k)
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) r.t[9 * k + 3 * i + j] = ja < jb ? tab[18 * p + 9 * k + 3 * i + j] : tab[18 * p + 9 * k + 3 * j + i];
        rows.push_back(r);
    }
    std::sort(rows.begin(), rows.end(), [](const Row& x, const Row& y) { return x.j1 != y.j1 ? x.j1 < y.j1 : x.j2 < y.j2; });
    rows.erase(std::unique(rows.begin(), rows.end(), [](const Row& x, const Row& y) { return x.j1 == y.j1 && x.j2 == y.j2; }), rows.end());
    const long long gap = ea.gapKb < 0.0 ? -1 : (long long)std::llround(ea.gapKb * 1000.0);
    unsigned long long screened = 0, written = 0, near = 0;
    for (const Row& r : rows) {
        if (gap >= 0 && bim.chr[r.j1] == bim.chr[r.j2] && std::llabs(bim.bp[r.j1] - bim.bp[r.j2]) <= gap) {
            ++near;
            continue;
        }
        ++screened;
        hgibbs_epi_result e{};
        hg_check(hgibbs_epi_test(r.t, &e), "hgibbs_epi_test");
        if (!(e.lr >= ea.chisq) || e.df <= 0) continue;
        long long n0 = 0, n1 = 0;
        for (int c = 0; c < 9; ++c) n0 += r.t[c], n1 += r.t[9 + c];
        std::fprintf(f, "%s\t%s\t%lld\t%s\t%s\t%lld\t%lld\t%lld\t%lld\t%.9g\t%.9g\t%d\t%.9g\t%d\n", bim.chr[r.j1].c_str(), bim.id[r.j1].c_str(), bim.bp[r.j1],
                     bim.chr[r.j2].c_str(), bim.id[r.j2].c_str(), bim.bp[r.j2], n0 + n1, n1, n0, e.ksa, e.lr, e.df, e.p, e.converged);
        ++written;
    }
    close_out(f, out);
    std::printf("EPISTASIS: %llu pairs tested (%zu listed markers without a finite sd left out), %llu screened in%s, %llu written to %s (%.3f ms of products, %.3f ms of screen on the device)\n",
                tested, dropped, screened, gap >= 0 ? (" (" + std::to_string(near) + " more within the gap)").c_str() : "", written, out.c_str(), pms, sms);
    return 0;
}

// ---- --sumstats: BayesR from a table of per-marker effects and the panel's LD band ----
// The table of --sumstats matched to the .bim by id: b_j = x_j'y on the chain's scale (xty), who takes part (use), and what was counted
struct SumstatTable {
    std::vector<double> xty;
    std::vector<uint8_t> use;
    double n_eff = 0.0;
    unsigned rows = 0, matched = 0, swapped = 0, unknown = 0, allele = 0, unusable = 0;
};

SumstatTable read_sumstats(const std::string& path, const BimRows& bim, unsigned M, const std::string& bimp, bool nGiven, double nOpt)
{
    std::ifstream in(path);
    if (!in) fatal("FATAL  : --sumstats: can not open the file [" + path + "] to read.");
    std::string line;
    if (!std::getline(in, line)) fatal("FATAL  : --sumstats: " + path + " has no header line");
    const std::vector<std::string> head = tokens(line, " \t\r");
    const char* const want[6] = {"SNP", "A1", "A2", "BETA", "SE", "N"};
    size_t col[6], last = 0;
    for (int w = 0; w < 6; ++w) {
        col[w] = head.size();
        for (size_t c = 0; c < head.size(); ++c)
            if (head[c] == want[w] && col[w] == head.size()) col[w] = c;
        if (col[w] == head.size())
            fatal("FATAL  : --sumstats: " + path + " has no column " + want[w] + " in its header line (it needs SNP A1 A2 BETA SE N, as --assoc writes them)");
        last = std::max(last, col[w]);
    }
    std::map<std::string, unsigned> at;
    for (unsigned j = 0; j < M; ++j)
        if (!at.emplace(bim.id[j], j).second) fatal("FATAL  : " + bimp + " lists SNP id " + bim.id[j] + " twice: --sumstats matches markers by id");
    SumstatTable t;
    t.xty.assign(M, 0.0);
    t.use.assign(M, 0);
    std::vector<double> z(M, 0.0), nj(M, 0.0), ns;
    std::map<std::string, unsigned> seen; // id -> line
    for (unsigned ln = 2; std::getline(in, line); ++ln) {
        const std::vector<std::string> tok = tokens(line, " \t\r");
        if (tok.empty()) continue;
        if (tok.size() <= last)
            fatal("FATAL  : --sumstats: " + path + " line " + std::to_string(ln) + " has " + std::to_string(tok.size()) + " columns, the header names " + std::to_string(head.size()));
        ++t.rows;
        const auto first = seen.emplace(tok[col[0]], ln);
        if (!first.second)
            fatal("FATAL  : --sumstats: " + path + " line " + std::to_string(ln) + ": SNP id " + tok[col[0]] + " was already on line " + std::to_string(first.first->second) + ": one row per marker");
        const auto hit = at.find(tok[col[0]]);
        if (hit == at.end()) {
            ++t.unknown;
            continue;
        }
        const unsigned j = hit->second;
        double sign = 1.0;
        if (tok[col[1]] == bim.a1[j] && tok[col[2]] == bim.a2[j]) sign = 1.0;
        else if (tok[col[1]] == bim.a2[j] && tok[col[2]] == bim.a1[j]) sign = -1.0; // the table counts the other allele
        else {
            ++t.allele;
            continue;
        }
        double b = 0.0, se = 0.0, n = 0.0;
        if (!whole_num(tok[col[3]], b) || !whole_num(tok[col[4]], se) || !whole_num(tok[col[5]], n) || !std::isfinite(b) || !std::isfinite(se) || !std::isfinite(n) ||
            !(se > 0.0) || !(n > 0.0)) { // NA, nan, a non-positive SE or N
            ++t.unusable;
            continue;
        }
        const double zz = b / se, den = n - 2.0 + zz * zz;
        if (!std::isfinite(zz) || !(den > 0.0)) {
            ++t.unusable;
            continue;
        }
        ++t.matched;
        t.swapped += sign < 0.0 ? 1u : 0u;
        t.use[j] = 1;
        z[j] = sign * zz;
        nj[j] = n;
        ns.push_back(n);
    }
    if (t.matched == 0) fatal("FATAL  : --sumstats: no row of " + path + " matches a marker of " + bimp + " (by SNP id and alleles) with usable BETA, SE and N");
    if (nGiven) t.n_eff = nOpt;
    else { // the median N of the matched rows (the mean of the two middle ones)
        std::sort(ns.begin(), ns.end());
        t.n_eff = ns.size() % 2 ? ns[ns.size() / 2] : 0.5 * (ns[ns.size() / 2 - 1] + ns[ns.size() / 2]);
    }
    if (!(t.n_eff >= 2.0)) fatal("FATAL  : --sumstats: n_eff = " + std::to_string(t.n_eff) + ": the sample size must be at least 2 (--sumstats-n sets it)");
    // the standardised effect z / sqrt(N_j - 2 + z^2) is x_j'y / (n - 1) for a y with y'y = n - 1
    for (unsigned j = 0; j < M; ++j)
        if (t.use[j]) t.xty[j] = (t.n_eff - 1.0) * (z[j] / std::sqrt(nj[j] - 2.0 + z[j] * z[j]));
    return t;
}

// --sumstats-post: which iterations are records, how many there are, and the table.
// `all`: every iteration at or after --burn-in (--sumstats-post-all), not only the thinned ones
bool post_counts(const Options& opt, unsigned iteration, bool all) { return iteration >= opt.burnin && (all || iteration % opt.thin == 0); }

unsigned post_records(const Options& opt, bool all)
{
    if (opt.burnin >= opt.chainLength) return 0;
    if (all || opt.thin <= 1) return opt.chainLength - opt.burnin;
    const unsigned first = (opt.burnin + opt.thin - 1) / opt.thin, last = (opt.chainLength - 1) / opt.thin; // multiples of --thin in [burn-in, length)
    return last >= first ? last - first + 1 : 0;
}

struct PostJob {
    bool on = false, only = false;
    unsigned T = 0;
    std::string path;
    const BimRows* bim = nullptr;
    const std::vector<double>* mstd = nullptr;
    const std::vector<uint8_t>* use = nullptr;
    int K = 0;
    double add_ms = 0.0, final_ms = 0.0; // device time of every add and of the table's kernel
};

PostJob post_job(const Options& opt, const std::string& base, const BimRows& bim, const std::vector<double>& mstd, const std::vector<uint8_t>& use, int K)
{
    PostJob p;
    p.on = opt.sumstatsPost;
    p.only = opt.sumstatsPostOnly;
    p.T = post_records(opt, opt.sumstatsPostAll);
    p.path = opt.sumstatsPostOut.empty() ? base + ".post" : opt.sumstatsPostOut;
    p.bim = &bim;
    p.mstd = &mstd;
    p.use = &use;
    p.K = K;
    return p;
}

// after the last record, while the chains' ss state still stands: the table of `chains` chains to p.path
void write_post_table(PostJob& p, hgibbs_t dev, unsigned chains, unsigned M)
{
    const int K = p.K;
    std::vector<double> mean(M), sd(M), pip(M), rhat(M);
    std::vector<uint32_t> cnt((size_t)K * M);
    hg_check(hgibbs_ss_post_get(dev, mean.data(), sd.data(), pip.data(), cnt.data(), rhat.data()), "hgibbs_ss_post_get");
    hg_check(hgibbs_last_ss_post_ms(dev, &p.add_ms, &p.final_ms), "hgibbs_last_ss_post_ms");
    hg_check(hgibbs_ss_post_end(dev), "hgibbs_ss_post_end");
    FILE* f = open_out(p.path, "wb+");
    std::fprintf(f, "CHR\tSNP\tBP\tA1\tA2\tUSED\tNCHAINS\tNREC\tMEAN\tSD\tBETA\tPIP");
    for (int k = 1; k < K; ++k) std::fprintf(f, "\tPC%d", k);
    std::fprintf(f, "\tRHAT\n");
    const double all = (double)chains * (double)p.T;
    for (unsigned j = 0; j < M; ++j) {
        const BimRows& b = *p.bim;
        std::fprintf(f, "%s\t%s\t%lld\t%s\t%s\t%d", b.chr[j].c_str(), b.id[j].c_str(), b.bp[j], b.a1[j].c_str(), b.a2[j].c_str(), (*p.use)[j] ? 1 : 0);
        if (!(*p.use)[j]) {
            for (int k = 0; k < K + 6; ++k) std::fprintf(f, "\tNA");
            std::fprintf(f, "\n");
            continue;
        }
        std::fprintf(f, "\t%u\t%u\t%.9g\t%.9g\t%.9g\t%.9g", chains, p.T, mean[j], sd[j], mean[j] * (*p.mstd)[j], pip[j]);
        for (int k = 1; k < K; ++k) std::fprintf(f, "\t%.9g", (double)cnt[(size_t)k * M + j] / all);
        if (std::isnan(rhat[j]))
            std::fprintf(f, "\tNA\n");
        else
            std::fprintf(f, "\t%.9g\n", rhat[j]);
    }
    close_out(f, p.path);
}

// what the closing SUMSTAT: line gains with --sumstats-post
std::string post_report(const PostJob& p)
{
    if (!p.on) return "";
    char b[512];
    std::snprintf(b, sizeof b, ", %u records per chain counted on the device into %s (%.3f ms for all adds, %.3f ms for the table's kernel)", p.T, p.path.c_str(), p.add_ms,
                  p.final_ms);
    return b;
}

// ---- local credible sets: what --sumstats-cs and --cs share ----
// The sub-options of a route under its prefix ("--sumstats-cs", "--cs"): refused by name where they do not parse
void check_cs_values(const std::string& prefix, const CsStrings& a)
{
    const struct { const char* opt; const std::string& t; const char* what; } unit[4] = {
        {"-r2", a.r2, "the threshold on r^2"},
        {"-alpha", a.alpha, "the sum of PIPs a set must reach"},
        {"-pep", a.pep, "the posterior existence probability a set must have"},
        {"-lead", a.lead, "the PIP a marker needs to lead a set"},
    };
    double v = 0.0;
    for (const auto& u : unit)
        if (!u.t.empty() && (!whole_num(u.t, v) || !(v > 0.0 && v <= 1.0)))
            fatal("FATAL  : " + prefix + u.opt + " " + u.t + ": " + u.what + " must be a number in (0, 1]");
    long k = 0;
    if (!a.maxSize.empty() && (!whole_int(a.maxSize, k) || k < 1 || k > 256))
        fatal("FATAL  : " + prefix + "-max-size " + a.maxSize + ": the largest set must be an integer from 1 to 256 markers (the most hgibbs_cs_sets takes)");
}

// a plan without a record: the history counts the thinned iterations at or after --burn-in
void check_cs_plan(const std::string& flag, const Options& opt)
{
    if (post_records(opt, false) == 0)
        fatal("FATAL  : " + flag + ": 0 records per chain (--chain-length " + std::to_string(opt.chainLength) + ", --burn-in " + std::to_string(opt.burnin) + ", --thin " +
              std::to_string(opt.thin) + "): the history needs a thinned iteration at or after the burn-in");
}

// x of NREC records as a count: at least 1
uint32_t cs_ceil(double x, uint64_t NREC) { return std::max<uint32_t>(1u, (uint32_t)std::ceil(x * (double)NREC)); }

struct CsJob {
    bool on = false;
    double r2 = 0.5, alpha = 0.9, pep = 0.7, lead = 0.01;
    uint32_t maxSize = 64;
    std::string path;
    uint32_t C = 1, T = 0; // the history's chains and records per chain
    // what the five steps found
    uint32_t nleads = 0, reached = 0, fell_short = 0, capped = 0, low_pep = 0, written = 0;
    double add_ms = 0.0, mask_ms = 0.0, sets_ms = 0.0;
};

CsJob cs_job(bool on, const CsStrings& a, const std::string& dflt_path)
{
    CsJob c;
    c.on = on;
    c.r2 = num_or(a.r2, 0.5);
    c.alpha = num_or(a.alpha, 0.9);
    c.pep = num_or(a.pep, 0.7);
    c.lead = num_or(a.lead, 0.01);
    long k = 64;
    if (!a.maxSize.empty()) whole_int(a.maxSize, k);
    c.maxSize = (uint32_t)k;
    c.path = a.out.empty() ? dflt_path : a.out;
    return c;
}

// the table of the accepted sets, in the order taken
void write_cs_table(FILE* f, const BimRows& bim, uint64_t NREC, const std::vector<uint32_t>& cnt, const std::vector<uint32_t>& leads, const std::vector<uint32_t>& size,
                    const std::vector<uint64_t>& sum, const std::vector<uint32_t>& pep, const std::vector<uint32_t>& members, uint32_t max_size,
                    const std::vector<uint32_t>& taken)
{
    std::fprintf(f, "CS\tLEAD\tCHR\tBP_FIRST\tBP_LAST\tSIZE\tNREC\tPIP_LEAD\tPIP_SUM\tPEP\tSNPS\tPIPS\n");
    const double all = (double)NREC;
    for (size_t k = 0; k < taken.size(); ++k) {
        const uint32_t i = taken[k], v = leads[i];
        const uint32_t* mem = &members[(size_t)i * max_size];
        long long first = bim.bp[v], last = bim.bp[v];
        for (uint32_t m = 0; m < size[i]; ++m) {
            first = std::min(first, bim.bp[mem[m]]);
            last = std::max(last, bim.bp[mem[m]]);
        }
        std::fprintf(f, "%zu\t%s\t%s\t%lld\t%lld\t%u\t%llu\t%.9g\t%.9g\t%.9g\t", k + 1, bim.id[v].c_str(), bim.chr[v].c_str(), first, last, size[i],
                     (unsigned long long)NREC, (double)cnt[v] / all, (double)sum[i] / all, (double)pep[i] / all);
        for (uint32_t m = 0; m < size[i]; ++m) std::fprintf(f, "%s%s", m ? "," : "", bim.id[mem[m]].c_str());
        std::fprintf(f, "\t");
        for (uint32_t m = 0; m < size[i]; ++m) std::fprintf(f, "%s%.9g", m ? "," : "", (double)cnt[mem[m]] / all);
        std::fprintf(f, "\n");
    }
}

// After the last add, while the handle stands: counts, leads, the LD mask on the run's window, the candidate sets, the walk, the table
void cs_finish(CsJob& c, hgibbs_t dev, const BimRows& bim, const LdWindow& win, uint32_t W, unsigned M, FILE* f)
{
    const uint64_t NREC = (uint64_t)c.C * c.T;
    std::vector<uint32_t> cnt(M);
    hg_check(hgibbs_cs_counts(dev, cnt.data()), "hgibbs_cs_counts");
    const uint32_t min_lead = cs_ceil(c.lead, NREC), need = cs_ceil(c.alpha, NREC), min_pep = cs_ceil(c.pep, NREC);
    std::vector<uint32_t> leads, lead_cnt;
    for (unsigned j = 0; j < M; ++j)
        if (cnt[j] >= min_lead) {
            leads.push_back(j);
            lead_cnt.push_back(cnt[j]);
        }
    const uint32_t nlead = (uint32_t)leads.size();
    const size_t nm = (size_t)M * ((W + 63u) / 64u);
    std::vector<uint64_t> fwd(nm), bwd(nm);
    hg_check(hgibbs_ld_mask(dev, W, win.ahead.data(), c.r2, fwd.data(), bwd.data(), nullptr), "hgibbs_ld_mask");
    double products_ms = 0.0, reduce_ms = 0.0;
    hg_check(hgibbs_last_ld_mask_ms(dev, &products_ms, &reduce_ms), "hgibbs_last_ld_mask_ms");
    c.mask_ms = products_ms + reduce_ms;
    std::vector<uint32_t> status(nlead), size(nlead), pep(nlead), members((size_t)nlead * c.maxSize), taken(nlead);
    std::vector<uint64_t> sum(nlead);
    hg_check(hgibbs_cs_sets(dev, W, fwd.data(), bwd.data(), nlead, leads.data(), need, c.maxSize, status.data(), size.data(), sum.data(), pep.data(), members.data()),
             "hgibbs_cs_sets");
    double counts_ms = 0.0;
    hg_check(hgibbs_last_cs_ms(dev, &c.add_ms, &counts_ms, &c.sets_ms), "hgibbs_last_cs_ms");
    hg_check(hgibbs_cs_end(dev), "hgibbs_cs_end");
    uint32_t ntaken = 0;
    hg_check(hgibbs_cs_select(M, nlead, leads.data(), lead_cnt.data(), status.data(), size.data(), pep.data(), members.data(), c.maxSize, min_pep, taken.data(), &ntaken),
             "hgibbs_cs_select");
    taken.resize(ntaken);
    c.nleads = nlead;
    for (uint32_t i = 0; i < nlead; ++i) {
        c.reached += status[i] == 0u;
        c.fell_short += status[i] == 1u;
        c.capped += status[i] == 2u;
        c.low_pep += status[i] == 0u && pep[i] < min_pep;
    }
    c.written = ntaken;
    write_cs_table(f, bim, NREC, cnt, leads, size, sum, pep, members, c.maxSize, taken);
    close_out(f, c.path);
}

// what the closing line gains with the credible sets
std::string cs_report(const CsJob& c, unsigned M)
{
    if (!c.on) return "";
    const uint64_t NREC = (uint64_t)c.C * c.T;
    char b[768];
    std::snprintf(b, sizeof b,
                  ", credible sets from %llu records: %u leads, %u candidates reached alpha, %u ran short, %u hit the cap of %u markers, %u below the PEP bound, %u sets written to %s "
                  "(history %llu bytes on the device; %.3f ms for all adds, %.3f ms for the LD mask, %.3f ms for the sets' kernel)",
                  (unsigned long long)NREC, c.nleads, c.reached, c.fell_short, c.capped, c.maxSize, c.low_pep, c.written, c.path.c_str(),
                  (unsigned long long)((NREC + 63u) / 64u * 8u * M), c.add_ms, c.mask_ms, c.sets_ms);
    return b;
}

// The chains of --sumstats as the driver's loop sees them: the R of a hydra_ss_multi (--sumstats-chains), or
// the one hydra_ss_chain as R = 1.
struct SsChainSet {
    hydra_ss_chain_t one = nullptr;
    hydra_ss_multi_t many = nullptr;
    uint32_t R = 1;
    void iterate() const { one ? hg_check(hydra_ss_chain_iterate(one), "hydra_ss_chain_iterate") : hg_check(hydra_ss_multi_iterate(many), "hydra_ss_multi_iterate"); }
    void state(uint32_t r, double* sigmaE, double* mu, double* sigmaG, int32_t* m0) const
    {
        one ? hg_check(hydra_ss_chain_state(one, sigmaE, mu, sigmaG, nullptr, m0, nullptr, nullptr), "hydra_ss_chain_state")
            : hg_check(hydra_ss_multi_state(many, r, sigmaE, mu, sigmaG, nullptr, m0, nullptr, nullptr), "hydra_ss_multi_state");
    }
    void effects(uint32_t r, double* beta, int32_t* comp, double* acum) const
    {
        one ? hg_check(hydra_ss_chain_effects(one, beta, comp, acum, nullptr), "hydra_ss_chain_effects")
            : hg_check(hydra_ss_multi_effects(many, r, beta, comp, acum, nullptr), "hydra_ss_multi_effects");
    }
    int csv_line(uint32_t r, unsigned iteration, char* buf, size_t len) const
    {
        return one ? hydra_ss_chain_csv_line(one, iteration, buf, len) : hydra_ss_multi_csv_line(many, r, iteration, buf, len);
    }
    void streams(uint32_t* S, uint32_t* bounds) const
    {
        one ? hg_check(hydra_ss_chain_streams(one, S, bounds, nullptr), "hydra_ss_chain_streams") : hg_check(hydra_ss_multi_streams(many, S, bounds, nullptr), "hydra_ss_multi_streams");
    }
    void destroy() const { one ? (void)hydra_ss_chain_destroy(one) : (void)hydra_ss_multi_destroy(many); }
};

// <base>.rhat: the convergence table over the thinned records at or after --burn-in, rec[r P + p] holding parameter p of chain r
// (sigmaG[g] per group, their sum, sigmaE, h2 as the .csv's ratio, m0, mu).  Returns the largest R^.
double write_rhat(const Options& opt, const std::string& rhatp, const std::vector<std::vector<double>>& rec, long R, int G)
{
    const int P = G + 5;
    double max_rhat = std::numeric_limits<double>::quiet_NaN();
    const unsigned T = (unsigned)rec[0].size();
    FILE* rf = open_out(rhatp, "wb+");
    std::fprintf(rf, "PARAM\tNCHAINS\tNREC\tMEAN\tSD\tRHAT\tESS\n");
    if (T < 4)
        std::printf("SUMSTAT: %s: %u thinned record(s) per chain at or after --burn-in %u, split-R^ needs at least 4: every statistic is NA\n", rhatp.c_str(), T,
                    opt.burnin);
    auto num = [](double v) {
        char b[40];
        if (std::isnan(v)) return std::string("NA");
        std::snprintf(b, sizeof b, "%.9g", v);
        return std::string(b);
    };
    std::vector<double> x((size_t)R * T);
    for (int p = 0; p < P; ++p) {
        const double nan = std::numeric_limits<double>::quiet_NaN();
        double mean = nan, sd = nan, rhat = nan, ess = nan;
        if (T >= 4) {
            for (long r = 0; r < R; ++r) std::copy(rec[(size_t)r * P + p].begin(), rec[(size_t)r * P + p].end(), x.begin() + (size_t)r * T);
            hg_check(hgibbs_mcmc_diag((uint32_t)R, T, x.data(), &mean, &sd, &rhat, &ess), "hgibbs_mcmc_diag");
            if (!std::isnan(rhat) && !(rhat <= max_rhat)) max_rhat = rhat;
        }
        std::string name = p < G ? "sigmaG[" + std::to_string(p) + "]" : std::string(p == G ? "sigmaG" : p == G + 1 ? "sigmaE" : p == G + 2 ? "h2" : p == G + 3 ? "m0" : "mu");
        std::fprintf(rf, "%s\t%ld\t%u\t%s\t%s\t%s\t%s\n", name.c_str(), R, T, num(mean).c_str(), num(sd).c_str(), num(rhat).c_str(), num(ess).c_str());
    }
    close_out(rf, rhatp);
    return max_rhat;
}

// --sumstats from its chain(s) down, on the band of `dev`.  --sumstats-chains R: R chains from the model `md` with the seeds
// md.seed + r in one launch per iteration, chain 0's files <base>.*, chain r's <base>.c<r>.*, and <base>.rhat; without it the one
// chain of md.seed and the single chain's wording of the RESULT and the closing lines.
void run_sumstats_chains(const Options& opt, hgibbs_t dev, const hydra_model_desc& md, const SumstatTable& tab, const LdWindow& win, uint32_t W, unsigned M, int G,
                         const std::string& base, PostJob& post, CsJob& csj, unsigned used, unsigned nosd)
{
    const bool many = opt.sumstatsChainsGiven;
    long R = 1, smax = 0;
    if (many) whole_int(opt.sumstatsChains, R);
    if (opt.sumstatsStreamsGiven) whole_int(opt.sumstatsStreams, smax);
    SsChainSet cs;
    cs.R = (uint32_t)R;
    if (many) {
        std::vector<uint32_t> seeds(R);
        for (long r = 0; r < R; ++r) seeds[r] = md.seed + (uint32_t)r; // hydra's rule for ranks
        hg_check(hydra_ss_multi_create(dev, &md, cs.R, seeds.data(), tab.n_eff, W, win.ahead.data(), tab.xty.data(), tab.use.data(), (uint32_t)smax, &cs.many),
                 "hydra_ss_multi_create");
    } else {
        hg_check(hydra_ss_chain_create(dev, &md, tab.n_eff, W, win.ahead.data(), tab.xty.data(), tab.use.data(), &cs.one), "hydra_ss_chain_create");
        if (smax) hg_check(hydra_ss_chain_set_streams(cs.one, (uint32_t)smax), "hydra_ss_chain_set_streams");
    }
    // independent LD blocks in parallel streams: the intervals come from the window, so they are known before the first sweep
    uint32_t streams = 0, largest = 0;
    cs.streams(&streams, nullptr);
    if (streams) {
        std::vector<uint32_t> bounds((size_t)streams + 1u);
        cs.streams(nullptr, bounds.data());
        for (uint32_t s = 0; s < streams; ++s) largest = std::max(largest, bounds[s + 1] - bounds[s]);
    }
    double band_ms = 0.0, sweep_ms = 0.0;
    hg_check(hgibbs_last_ss_ms(dev, &band_ms, &sweep_ms), "hgibbs_last_ss_ms");
    if (post.on) hg_check(hgibbs_ss_post_begin(dev, many ? cs.R : 0u, post.T), "hgibbs_ss_post_begin"); // (0: the handle's own chain)
    if (csj.on) { // the thinned iterations at or after --burn-in, whatever --sumstats-post-all says
        csj.C = cs.R;
        csj.T = post_records(opt, false);
        hg_check(hgibbs_cs_begin(dev, csj.C, csj.T), "hgibbs_cs_begin");
    }
    const bool effects = !(post.on && post.only); // --sumstats-post-only: no .bet, .cpn, .acu, and no download of a record

    // the chains' files and formats (:1302-1309, :2736-2794)
    OutFiles outs;
    std::vector<FILE*> outf(R), betf(R), cpnf(R), acuf(R);
    for (long r = 0; r < R; ++r) {
        const std::string b = r ? base + ".c" + std::to_string(r) : base;
        outf[r] = outs.open(b + ".csv");
        if (!effects) continue;
        betf[r] = outs.open(b + ".bet");
        cpnf[r] = outs.open(b + ".cpn");
        acuf[r] = outs.open(b + ".acu");
        for (FILE* f : {betf[r], cpnf[r], acuf[r]}) pwrite_at(f, 0, &M, sizeof(unsigned));
    }
    const int P = G + 5; // the .rhat table's parameters; per chain its records in order
    std::vector<std::vector<double>> rec(many ? (size_t)P * R : 0);
    std::vector<double> beta(M), acum(M), sigmaG(G);
    std::vector<int32_t> comp(M), m0(G);
    std::vector<char> buff(50000);
    unsigned n_thinned_saved = 0, sweeps = 0;
    double sweep_total_ms = 0.0;
    for (unsigned iteration = 0; iteration < opt.chainLength; ++iteration) {
        const double t0 = now_s();
        cs.iterate();
        const double t1 = now_s();
        hg_check(hgibbs_last_ss_ms(dev, &band_ms, &sweep_ms), "hgibbs_last_ss_ms");
        sweep_total_ms += sweep_ms;
        ++sweeps;
        if (post.on && post_counts(opt, iteration, opt.sumstatsPostAll)) hg_check(hgibbs_ss_post_add(dev), "hgibbs_ss_post_add");
        if (csj.on && post_counts(opt, iteration, false)) hg_check(hgibbs_ss_cs_add(dev, many ? cs.R : 0u), "hgibbs_ss_cs_add");
        for (long r = 0; r < R; ++r) {
            double sigmaE = 0, mu = 0;
            cs.state((uint32_t)r, &sigmaE, &mu, sigmaG.data(), m0.data());
            double sg = 0;
            long m0s = 0;
            for (int g = 0; g < G; ++g) {
                sg += sigmaG[g];
                m0s += m0[g];
            }
            if (many)
                std::printf("RESULT : chain %2ld it %4d: proc = %9.3f s (all chains), sweep = %9.3f ms on the device (all chains), sigmaG = %15.10f, sigmaE = %15.10f, "
                            "mu = %15.10f, m0 = %10ld\n",
                            r, iteration, t1 - t0, sweep_ms, sg, sigmaE, mu, m0s);
            else
                std::printf("RESULT : it %4d: proc = %9.3f s, sweep = %9.3f ms on the device, sigmaG = %15.10f, sigmaE = %15.10f, mu = %15.10f, m0 = %10ld\n", iteration,
                            t1 - t0, sweep_ms, sg, sigmaE, mu, m0s);
            if (iteration % opt.thin != 0) continue;
            if (effects) cs.effects((uint32_t)r, beta.data(), comp.data(), acum.data());
            const int len = cs.csv_line((uint32_t)r, iteration, buff.data(), buff.size());
            write_line(outf[r], n_thinned_saved, buff.data(), len);
            if (effects) {
                write_thinned(betf[r], n_thinned_saved, iteration, beta.data(), M, sizeof(double));
                write_thinned(acuf[r], n_thinned_saved, iteration, acum.data(), M, sizeof(double));
                write_thinned(cpnf[r], n_thinned_saved, iteration, comp.data(), M, sizeof(int));
            }
            if (many && iteration >= opt.burnin) {
                std::vector<double>* row = &rec[(size_t)r * P];
                for (int g = 0; g < G; ++g) row[g].push_back(sigmaG[g]);
                row[G].push_back(sg);
                row[G + 1].push_back(sigmaE);
                row[G + 2].push_back(sg / (sigmaE + sg));
                row[G + 3].push_back((double)m0s);
                row[G + 4].push_back(mu);
            }
        }
        std::fflush(stdout);
        if (iteration % opt.thin == 0) n_thinned_saved += 1;
    }
    outs.close(true);
    if (post.on) write_post_table(post, dev, cs.R, M);
    if (csj.on) cs_finish(csj, dev, *post.bim, win, W, M, open_out(csj.path, "wb+"));
    cs.destroy();
    const double max_rhat = many ? write_rhat(opt, base + ".rhat", rec, R, G) : 0.0;
    hgibbs_destroy(dev);

    const char* files = post.on && post.only ? "csv" : "{csv,bet,cpn,acu}";
    char par[96] = "", rh[48] = "NA";
    if (streams) std::snprintf(par, sizeof par, " in %u streams (largest interval %u markers)", streams, largest);
    if (!std::isnan(max_rhat)) std::snprintf(rh, sizeof rh, "%.9g", max_rhat);
    std::printf("SUMSTAT: %u markers used, %u left out (%u not in the table, %u with another allele pair, %u without usable BETA, SE and N, %u without a finite sd in the panel), "
                "n_eff %.12g, band %u x %u doubles = %.1f MiB of device memory (built in %.3f ms), ",
                used, M - used, M - tab.matched - tab.allele - tab.unusable, tab.allele, tab.unusable, nosd, tab.n_eff, M, W, (double)M * W * 8.0 / 1048576.0, band_ms);
    const double per_sweep = sweeps ? sweep_total_ms / sweeps : 0.0;
    if (many)
        std::printf("%u chains, %.3f ms per sweep launch (all chains) on the device over %u sweeps%s, largest R^ %s, wrote %s.%s, %s.c<r>.%s for the chains r >= 1 and %s.rhat%s\n",
                    cs.R, per_sweep, sweeps, par, rh, base.c_str(), files, base.c_str(), files, base.c_str(), (post_report(post) + cs_report(csj, M)).c_str());
    else
        std::printf("%.3f ms per sweep on the device over %u sweeps%s, wrote %s.%s%s\n", per_sweep, sweeps, par, base.c_str(), files, (post_report(post) + cs_report(csj, M)).c_str());
}

// ---- --cs: the credible sets of a finished chain, from its .bet records ----
int run_cs(const Options& opt, const Cohort& co)
{
    const std::string base = opt.mcmcOutDir + "/" + opt.mcmcOutNam;
    const std::string bimp = opt.bedFile + ".bim";
    const unsigned M = co.Mtot;
    const BimRows bim = read_bim(bimp, M);
    long R = 1;
    if (!opt.csChains.empty()) whole_int(opt.csChains, R);

    // the pooled records at or after --burn-in: a marker is in the model iff its effect is not 0
    std::vector<unsigned> its;
    std::vector<double> betas;
    for (long r = 0; r < R; ++r) {
        const size_t before = its.size();
        const std::string path = (r ? base + ".c" + std::to_string(r) : base) + ".bet";
        read_bet_records(path, M, opt.burnin, its, betas, "--cs takes the inclusion history from the chain's effects");
        if (its.size() == before) fatal("FATAL  : " + path + ": no record at or after --burn-in " + std::to_string(opt.burnin));
    }
    const size_t total = its.size();
    if (total >= (1ull << 32)) fatal("FATAL  : --cs: " + std::to_string(total) + " records, the history takes fewer than 2^32");

    // the window: kilobases (1000 unless markers are asked for), an index interval per chromosome
    const bool bySnps = opt.csSnpsGiven;
    long wsnps = 0;
    if (bySnps) whole_int(opt.csSnps, wsnps);
    const long long maxbp = (long long)std::llround(1000.0 * num_or(opt.csKb, 1000.0));
    const LdWindow win = ld_window("--cs", "hgibbs_ld_mask", bim, bimp, M, bySnps, wsnps, maxbp, "--cs-window-snps");
    const uint32_t W = std::max(1u, win.widest);

    CsJob csj = cs_job(true, opt.csArgs, base + ".cs");
    csj.C = 1;
    csj.T = (uint32_t)total;
    std::printf("CS     : %zu records at or after --burn-in %u from %ld chain(s) of %s, window %s, %llu pairs in the window, widest window %u markers ahead, r^2 >= %g -> %s\n",
                total, opt.burnin, R, base.c_str(), win.what.c_str(), win.npairs, win.widest, csj.r2, csj.path.c_str());
    std::fflush(stdout);

    std::vector<uint8_t> bed = read_training(opt.bedFile, co.numInds, M);
    if (opt.csArgs.out.empty()) make_out_dir(opt);
    FILE* f = open_out(csj.path, "wb+");

    hgibbs_t dev = open_training(co, bed);
    hg_check(hgibbs_cs_begin(dev, csj.C, csj.T), "hgibbs_cs_begin");
    std::vector<uint8_t> flags(M);
    for (size_t q = 0; q < total; ++q) {
        const double* b = &betas[q * M];
        for (unsigned j = 0; j < M; ++j) flags[j] = b[j] != 0.0 ? 1 : 0;
        hg_check(hgibbs_cs_add_flags(dev, flags.data()), "hgibbs_cs_add_flags");
    }
    cs_finish(csj, dev, bim, win, W, M, f);
    hgibbs_destroy(dev);
    std::printf("CS     : %u markers%s\n", M, cs_report(csj, M).c_str());
    return 0;
}

int run_sumstats(const Options& opt, const Cohort& co, const std::vector<int32_t>& groups, const std::vector<double>& mS_flat, int G, int K)
{
    const std::string base = opt.mcmcOutDir + "/" + opt.mcmcOutNam;
    const std::string bimp = opt.bedFile + ".bim";
    const unsigned M = co.Mtot;
    const BimRows bim = read_bim(bimp, M);

    // the window: kilobases (1000 unless markers are asked for), an index interval per chromosome
    const bool bySnps = opt.sumstatsWindowGiven;
    long wsnps = 0;
    if (bySnps) whole_int(opt.sumstatsWindow, wsnps);
    const long long maxbp = (long long)std::llround(1000.0 * num_or(opt.sumstatsKb, 1000.0));
    const LdWindow win = ld_window("--sumstats", "hgibbs_ss_begin", bim, bimp, M, bySnps, wsnps, maxbp, "--sumstats-window");
    const uint32_t W = std::max(1u, win.widest);

    double nOpt = 0.0;
    if (opt.sumstatsNGiven) whole_num(opt.sumstatsN, nOpt);
    SumstatTable tab = read_sumstats(opt.sumstatsFile, bim, M, bimp, opt.sumstatsNGiven, nOpt);
    std::printf("SUMSTAT: %u rows read from %s, %u matched to the .bim (%u with swapped alleles, sign flipped), %u ids not in it, %u with another allele pair, "
                "%u without usable BETA, SE and N; n_eff %.12g (%s); window %s, %llu pairs in the window, widest window %u markers ahead\n",
                tab.rows, opt.sumstatsFile.c_str(), tab.matched, tab.swapped, tab.unknown, tab.allele, tab.unusable, tab.n_eff,
                opt.sumstatsNGiven ? "--sumstats-n" : "the median N of the matched rows", win.what.c_str(), win.npairs, win.widest);
    std::fflush(stdout);

    std::vector<uint8_t> bed = read_training(opt.bedFile, co.numInds, M);
    make_out_dir(opt);
    hgibbs_t dev = open_training(co, bed);
    std::vector<double> mstd(M);
    hg_check(hgibbs_marker_stats(dev, nullptr, mstd.data(), nullptr, nullptr, nullptr), "hgibbs_marker_stats");
    unsigned nosd = 0, used = 0;
    for (unsigned j = 0; j < M; ++j) {
        if (tab.use[j] && !std::isfinite(mstd[j])) {
            tab.use[j] = 0;
            tab.xty[j] = 0.0;
            ++nosd;
        }
        used += tab.use[j];
    }
    if (used == 0) fatal("FATAL  : --sumstats: every matched marker lacks a finite standard deviation in the panel");

    hydra_model_desc md{};
    md.seed = opt.seed;
    md.shuffle = opt.shuffleMarkers;
    md.G = G;
    md.K = K;
    md.groups = groups.empty() ? nullptr : groups.data();
    md.mS = mS_flat.data();
    PostJob post = post_job(opt, base, bim, mstd, tab.use, K);
    CsJob csj = cs_job(opt.sumstatsCs, opt.ssCs, base + ".cs");
    run_sumstats_chains(opt, dev, md, tab, win, W, M, G, base, post, csj, used, nosd);
    return 0;
}

// ---- the analysis modes -------------------------------------------------------
// An analysis mode is an option that, appended to a bayesMPI command line, samples nothing and runs one analysis on the chain's rows
// (run_predict .. run_qc above).  What the modes share is refused in one place, from one row per mode.
struct Mode {
    const char* flag;   // the option that asks for the mode
    bool given;
    const char* wmpi;   // how it refuses --mpibayes bayesWMPI, after its flag
    const char* orphan; // the first of its dependent options that was given: they need the mode (null: none was)
};
enum { PREDICT, LD, ASSOC, KING, PCA, PVE, GRM, LDSCORE, CLUMP, LDPRUNE, HE, QC, HOMOZYG, EPISTASIS, CS, REML, NMODES }; // the order in which a mode names the earlier ones it cannot be combined with

const char* first_given(std::initializer_list<std::pair<const char*, bool>> deps)
{
    for (const auto& d : deps)
        if (d.second) return d.first;
    return nullptr;
}

// the modes' own arguments
void check_ld_args(const Options& opt)
{
    if (opt.ldWindow < 1 || opt.ldWindow > 4096)
        fatal("FATAL  : --ld-window " + std::to_string(opt.ldWindow) + ": the window must be 1 to 4096 markers (the widest hgibbs_ld takes)");
    if (!(opt.ldWindowR2 >= 0.0 && opt.ldWindowR2 <= 1.0)) fatal("FATAL  : --ld-window-r2 must be in [0, 1]");
    if (opt.ldKbGiven && !(opt.ldWindowKb >= 0.0)) fatal("FATAL  : --ld-window-kb must not be negative");
}

void check_assoc_args(const Options& opt)
{
    if (!opt.assocLogistic)
        if (const char* o = first_given({{"--assoc-spa", opt.assocSpa}, {"--assoc-spa-sd", opt.assocSpaSdGiven}, {"--assoc-firth", opt.assocFirth},
                                         {"--assoc-firth-p", opt.assocFirthPGiven}}))
            fatal(std::string("FATAL  : ") + o + " needs --assoc-logistic");
    if (opt.assocSpaSdGiven && !opt.assocSpa) fatal("FATAL  : --assoc-spa-sd needs --assoc-spa");
    double t = 0.0;
    if (opt.assocSpaSdGiven && (!whole_num(opt.assocSpaSd, t) || !std::isfinite(t) || !(t >= 0.1)))
        fatal("FATAL  : --assoc-spa-sd " + opt.assocSpaSd + ": the threshold must be a finite number of standard deviations >= 0.1 (the saddlepoint formula divides by a quantity that goes to 0 with the score)");
    if (opt.assocFirthPGiven && !opt.assocFirth) fatal("FATAL  : --assoc-firth-p needs --assoc-firth");
    if (opt.assocFirth && opt.assocSpa) fatal("FATAL  : --assoc-firth with --assoc-spa: choose one correction (each writes its own P)");
    if (opt.assocFirthPGiven && (!whole_num(opt.assocFirthP, t) || !std::isfinite(t) || !(t > 0.0 && t <= 1.0)))
        fatal("FATAL  : --assoc-firth-p " + opt.assocFirthP + ": the threshold must be a finite number in (0, 1] (the score-test P at or below which a marker is refitted)");
    if (opt.assocSets.empty())
        if (const char* o = first_given({{"--assoc-set-beta", opt.assocSetBetaGiven}, {"--assoc-set-maf", opt.assocSetMafGiven}, {"--assoc-set-out", !opt.assocSetOut.empty()}}))
            fatal(std::string("FATAL  : ") + o + " needs --assoc-sets");
    if (!opt.assocSets.empty() && !opt.assocLogistic)
        fatal("FATAL  : --assoc-sets needs --assoc-logistic (the set tests of the linear model are not built)");
}

void check_king_args(const Options& opt)
{
    double t = 0.0;
    if (!whole_num(opt.kingCutoff, t) || !std::isfinite(t)) fatal("FATAL  : --king-cutoff " + opt.kingCutoff + ": the cutoff must be a finite number");
}

void check_pca_args(const Options& opt)
{
    long v = 0;
    double t = 0.0;
    if (!whole_int(opt.pcaK, v) || v < 1 || v > PCA_KMAX)
        fatal("FATAL  : --pca " + opt.pcaK + ": the number of components must be an integer from 1 to " + std::to_string(PCA_KMAX));
    if (opt.pcaItersGiven && (!whole_int(opt.pcaIters, v) || v < 1)) fatal("FATAL  : --pca-iters " + opt.pcaIters + ": needs at least one iteration");
    if (opt.pcaItersGiven && v > std::numeric_limits<int>::max())
        fatal("FATAL  : --pca-iters " + opt.pcaIters + ": at most " + std::to_string(std::numeric_limits<int>::max()) + " iterations");
    if (opt.pcaTolGiven && (!whole_num(opt.pcaTol, t) || !std::isfinite(t) || t < 0.0))
        fatal("FATAL  : --pca-tol " + opt.pcaTol + ": the tolerance must be a finite number >= 0");
}

void check_grm_args(const Options& opt)
{
    double t = 0.0;
    if (opt.grmSparseGiven && (!whole_num(opt.grmSparse, t) || !std::isfinite(t)))
        fatal("FATAL  : --grm-sparse " + opt.grmSparse + ": the cutoff must be a finite number");
}

void check_ldscore_args(const Options& opt)
{
    if (opt.ldScoreKbGiven && opt.ldScoreSnpsGiven) fatal("FATAL  : --ld-score-kb cannot be combined with --ld-score-snps: one way to define the window");
    if (!opt.ldScoreSets.empty() && opt.ldScoreGroups)
        fatal("FATAL  : --ld-score-sets cannot be combined with --ld-score-groups: one way to define the annotations");
    long w = 0;
    double t = 0.0;
    if (opt.ldScoreKbGiven && (!whole_num(opt.ldScoreKb, t) || !std::isfinite(t) || t < 0.0))
        fatal("FATAL  : --ld-score-kb " + opt.ldScoreKb + ": the window must be a finite number of kilobases >= 0");
    if (opt.ldScoreSnpsGiven && (!whole_int(opt.ldScoreSnps, w) || w < 1 || w > 4096))
        fatal("FATAL  : --ld-score-snps " + opt.ldScoreSnps + ": the window must be an integer from 1 to 4096 markers (the widest hgibbs_ld_scores takes)");
    if (opt.ldScoreGroups && opt.groupIndexFile.empty()) fatal("FATAL  : --ld-score-groups needs --groupIndexFile");
}

// a threshold of --clump or --ld-prune: a number as a whole, in [0, 1]
void check_unit(const char* flag, const std::string& t, const char* what)
{
    double v = 0.0;
    if (!t.empty() && (!whole_num(t, v) || !(v >= 0.0 && v <= 1.0))) fatal(std::string("FATAL  : ") + flag + " " + t + ": " + what + " must be a number in [0, 1]");
}

// the window options of --clump and --ld-prune
void check_ldselect_window(const std::string& flag, bool kbGiven, const std::string& kb, bool snpsGiven, const std::string& snps)
{
    if (kbGiven && snpsGiven) fatal("FATAL  : " + flag + "-kb cannot be combined with " + flag + "-snps: one way to define the window");
    long w = 0;
    double t = 0.0;
    if (kbGiven && (!whole_num(kb, t) || !std::isfinite(t) || t < 0.0)) fatal("FATAL  : " + flag + "-kb " + kb + ": the window must be a finite number of kilobases >= 0");
    if (snpsGiven && (!whole_int(snps, w) || w < 1 || w > 4096))
        fatal("FATAL  : " + flag + "-snps " + snps + ": the window must be an integer from 1 to 4096 markers (the widest hgibbs_ld_mask takes)");
}

void check_clump_args(const Options& opt)
{
    check_unit("--clump-p1", opt.clumpP1, "the P a marker needs to lead a clump");
    check_unit("--clump-p2", opt.clumpP2, "the P a marker needs to take part");
    check_unit("--clump-r2", opt.clumpR2, "the threshold on r^2");
    double p1 = 1e-4, p2 = 1e-2;
    if (!opt.clumpP1.empty()) whole_num(opt.clumpP1, p1);
    if (!opt.clumpP2.empty()) whole_num(opt.clumpP2, p2);
    if (p2 < p1)
        fatal("FATAL  : --clump-p2 " + (opt.clumpP2.empty() ? std::string("0.01") : opt.clumpP2) + " is below --clump-p1 " +
              (opt.clumpP1.empty() ? std::string("0.0001") : opt.clumpP1) + ": a marker that may lead a clump must take part");
    check_ldselect_window("--clump", opt.clumpKbGiven, opt.clumpKb, opt.clumpSnpsGiven, opt.clumpSnps);
}

void check_ldprune_args(const Options& opt)
{
    if (opt.ldPruneT.empty()) fatal("FATAL  : --ld-prune : the threshold on r^2 must be a number in [0, 1]");
    check_unit("--ld-prune", opt.ldPruneT, "the threshold on r^2");
    check_ldselect_window("--ld-prune", opt.ldPruneKbGiven, opt.ldPruneKb, opt.ldPruneSnpsGiven, opt.ldPruneSnps);
}

void check_pve_args(const Options& opt)
{
    const char* const definer[4] = {"--pve-window-kb", "--pve-window-snps", "--pve-sets", "--pve-groups"};
    const bool given[4] = {opt.pveKbGiven, opt.pveSnpsGiven, !opt.pveSets.empty(), opt.pveGroups};
    for (int x = 0; x < 4; ++x)
        for (int y = x + 1; y < 4; ++y)
            if (given[x] && given[y]) fatal(std::string("FATAL  : ") + definer[x] + " cannot be combined with " + definer[y] + ": one way to define the sets");
    long w = 0;
    double t = 0.0;
    if (opt.pveKbGiven && (!whole_num(opt.pveKb, t) || !std::isfinite(t) || !(t > 0.0)))
        fatal("FATAL  : --pve-window-kb " + opt.pveKb + ": the window must be a finite number of kilobases > 0");
    if (opt.pveSnpsGiven && (!whole_int(opt.pveSnps, w) || w < 1)) fatal("FATAL  : --pve-window-snps " + opt.pveSnps + ": the window must be an integer >= 1");
    if (opt.pveThresholdGiven && (!whole_num(opt.pveThreshold, t) || !std::isfinite(t) || t < 0.0 || t >= 1.0))
        fatal("FATAL  : --pve-threshold " + opt.pveThreshold + ": the threshold must be a finite number in [0, 1)");
    if (opt.pveGroups && opt.groupIndexFile.empty()) fatal("FATAL  : --pve-groups needs --groupIndexFile");
}

void check_qc_args(const Options& opt)
{
    struct { const char* flag; bool given; const std::string& t; double lo, hi; const char* what; } const unit[4] = {
        {"--qc-maf", opt.qcMafGiven, opt.qcMaf, 0.0, 0.5, "the minor allele frequency must be a number in [0, 0.5]"},
        {"--qc-geno", opt.qcGenoGiven, opt.qcGeno, 0.0, 1.0, "the missing rate of a marker must be a number in [0, 1]"},
        {"--qc-mind", opt.qcMindGiven, opt.qcMind, 0.0, 1.0, "the missing rate of an individual must be a number in [0, 1]"},
        {"--qc-hwe", opt.qcHweGiven, opt.qcHwe, 0.0, 1.0, "the P value must be a number in [0, 1]"},
    };
    double v = 0.0;
    for (const auto& u : unit)
        if (u.given && (!whole_num(u.t, v) || !(v >= u.lo && v <= u.hi))) fatal(std::string("FATAL  : ") + u.flag + " " + u.t + ": " + u.what);
    if (opt.qcHetSdGiven && (!whole_num(opt.qcHetSd, v) || !std::isfinite(v) || !(v > 0.0)))
        fatal("FATAL  : --qc-het-sd " + opt.qcHetSd + ": the number of standard deviations must be a finite number > 0");
}

void check_cs_args(const Options& opt)
{
    long r = 0;
    if (!opt.csChains.empty() && (!whole_int(opt.csChains, r) || r < 1 || r > 64))
        fatal("FATAL  : --cs-chains " + opt.csChains + ": the number of chains must be an integer from 1 to 64 (the most --sumstats-chains writes)");
    check_ldselect_window("--cs-window", opt.csKbGiven, opt.csKb, opt.csSnpsGiven, opt.csSnps);
    check_cs_values("--cs", opt.csArgs);
    check_cs_plan("--cs", opt);
}

void check_homozyg_args(const Options& opt)
{
    (void)homozyg_args(opt); // refuses by name what is out of range
}

// Every refusal of the modes, before anything is read: mode by mode (--ld-window first, then in the table's order), what all share,
// then the mode's own arguments
void check_modes(const Options& opt, int nranks)
{
    const char* const takes = "takes a bayesMPI command line, not --mpibayes bayesWMPI";
    const Mode modes[NMODES] = {
        {"--predict-bfile", !opt.predictBfile.empty(), "scores with bayesMPI effects only, not with --mpibayes bayesWMPI",
         first_given({{"--predict-dry-run", opt.predictDryRun}, {"--predict-out", !opt.predictOut.empty()}})},
        {"--ld-window", opt.ldGiven, takes,
         first_given({{"--ld-out", !opt.ldOut.empty()}, {"--ld-window-kb", opt.ldKbGiven}, {"--ld-window-r2", opt.ldR2Given}, {"--ld-bin", opt.ldBin}})},
        {"--assoc", opt.assoc, takes, first_given({{"--assoc-out", !opt.assocOut.empty()}, {"--assoc-no-loco", opt.assocNoLoco}, {"--assoc-logistic", opt.assocLogistic},
                                                   {"--assoc-spa", opt.assocSpa}, {"--assoc-spa-sd", opt.assocSpaSdGiven},
                                                   {"--assoc-firth", opt.assocFirth}, {"--assoc-firth-p", opt.assocFirthPGiven},
                                                   {"--assoc-sets", !opt.assocSets.empty()}, {"--assoc-set-beta", opt.assocSetBetaGiven},
                                                   {"--assoc-set-maf", opt.assocSetMafGiven}, {"--assoc-set-out", !opt.assocSetOut.empty()}})},
        {"--king", opt.king, takes, first_given({{"--king-out", !opt.kingOut.empty()}, {"--king-cutoff", opt.kingCutoffGiven}})},
        {"--pca", opt.pca, takes,
         first_given({{"--pca-iters", opt.pcaItersGiven}, {"--pca-tol", opt.pcaTolGiven}, {"--pca-out", opt.pcaOutGiven}, {"--pca-loadings", opt.pcaLoadings}})},
        {"--pve", opt.pve, takes,
         first_given({{"--pve-window-kb", opt.pveKbGiven}, {"--pve-window-snps", opt.pveSnpsGiven}, {"--pve-sets", !opt.pveSets.empty()}, {"--pve-groups", opt.pveGroups},
                      {"--pve-threshold", opt.pveThresholdGiven}, {"--pve-out", !opt.pveOut.empty()}, {"--pve-bin", opt.pveBin}})},
        {"--grm", opt.grm, takes, first_given({{"--grm-out", !opt.grmOut.empty()}, {"--grm-sparse", opt.grmSparseGiven}})},
        {"--ld-score", opt.ldScore, takes,
         first_given({{"--ld-score-kb", opt.ldScoreKbGiven}, {"--ld-score-snps", opt.ldScoreSnpsGiven}, {"--ld-score-sets", !opt.ldScoreSets.empty()},
                      {"--ld-score-groups", opt.ldScoreGroups}, {"--ld-score-raw", opt.ldScoreRaw}, {"--ld-score-out", !opt.ldScoreOut.empty()}})},
        {"--clump", opt.clump, takes,
         first_given({{"--clump-p1", !opt.clumpP1.empty()}, {"--clump-p2", !opt.clumpP2.empty()}, {"--clump-r2", !opt.clumpR2.empty()}, {"--clump-kb", opt.clumpKbGiven},
                      {"--clump-snps", opt.clumpSnpsGiven}, {"--clump-snp-field", !opt.clumpSnpField.empty()}, {"--clump-field", !opt.clumpField.empty()},
                      {"--clump-out", !opt.clumpOut.empty()}})},
        {"--ld-prune", opt.ldPrune, takes,
         first_given({{"--ld-prune-kb", opt.ldPruneKbGiven}, {"--ld-prune-snps", opt.ldPruneSnpsGiven}, {"--ld-prune-out", !opt.ldPruneOut.empty()}})},
        {"--he", opt.he, takes, first_given({{"--he-out", !opt.heOut.empty()}, {"--he-rows", opt.heRows}})},
        {"--qc", opt.qc, takes,
         first_given({{"--qc-out", !opt.qcOut.empty()}, {"--qc-maf", opt.qcMafGiven}, {"--qc-geno", opt.qcGenoGiven}, {"--qc-mind", opt.qcMindGiven},
                      {"--qc-hwe", opt.qcHweGiven}, {"--qc-het-sd", opt.qcHetSdGiven}})},
        {"--homozyg", opt.homozyg, takes,
         first_given({{"--homozyg-window-snp", !opt.hzWindow.empty()}, {"--homozyg-window-het", !opt.hzWindowHet.empty()},
                      {"--homozyg-window-missing", !opt.hzWindowMissing.empty()}, {"--homozyg-window-threshold", !opt.hzThreshold.empty()},
                      {"--homozyg-snp", !opt.hzSnp.empty()}, {"--homozyg-kb", !opt.hzKb.empty()}, {"--homozyg-density", !opt.hzDensity.empty()},
                      {"--homozyg-gap", !opt.hzGap.empty()}, {"--homozyg-het", !opt.hzHet.empty()}, {"--homozyg-out", !opt.hzOut.empty()}})},
        {"--epistasis", opt.epistasis, takes,
         first_given({{"--epistasis-chisq", !opt.epiChisq.empty()}, {"--epistasis-sets", !opt.epiSets.empty()}, {"--epistasis-gap", !opt.epiGap.empty()},
                      {"--epistasis-out", !opt.epiOut.empty()}})},
        {"--cs", opt.cs, takes,
         first_given({{"--cs-chains", !opt.csChains.empty()}, {"--cs-window-kb", opt.csKbGiven}, {"--cs-window-snps", opt.csSnpsGiven}, {"--cs-r2", !opt.csArgs.r2.empty()},
                      {"--cs-alpha", !opt.csArgs.alpha.empty()}, {"--cs-pep", !opt.csArgs.pep.empty()}, {"--cs-lead", !opt.csArgs.lead.empty()},
                      {"--cs-max-size", !opt.csArgs.maxSize.empty()}, {"--cs-out", !opt.csArgs.out.empty()}})},
        {"--reml", opt.reml, takes,
         first_given({{"--reml-trials", !opt.remlTrials.empty()}, {"--reml-h2-start", !opt.remlH2.empty()}, {"--reml-cg-tol", !opt.remlCgTol.empty()},
                      {"--reml-cg-iters", !opt.remlCgIters.empty()}, {"--reml-tol", !opt.remlTol.empty()}, {"--reml-out", !opt.remlOut.empty()},
                      {"--reml-blup", opt.remlBlup}})},
    };
    for (const int i : {LD, PREDICT, ASSOC, KING, PCA, PVE, GRM, LDSCORE, CLUMP, LDPRUNE, HE, QC, HOMOZYG, EPISTASIS, CS, REML}) {
        const Mode& m = modes[i];
        const std::string flag = m.flag;
        if (!m.given) {
            if (m.orphan) fatal(std::string("FATAL  : ") + m.orphan + " needs " + flag);
            continue;
        }
        if (opt.bayesType == "bayesWMPI") fatal("FATAL  : " + flag + " " + m.wmpi);
        if (opt.bedFile.empty())
            fatal("FATAL  : " + flag + " needs --bfile: its .fam and .bim name the rows and the markers (the genotypes may still come from --sparse-dir/--sparse-basename)");
        for (int j = 0; j < i; ++j)
            if (modes[j].given) fatal("FATAL  : " + flag + " cannot be combined with " + modes[j].flag);
        if (opt.restart) fatal("FATAL  : " + flag + " does not sample: it cannot be combined with --restart");
        if (nranks > 1) fatal("FATAL  : " + flag + " runs on one process (WORLD_SIZE = " + std::to_string(nranks) + ")");
        if (i == LD) check_ld_args(opt);
        if (i == ASSOC) check_assoc_args(opt);
        if (i == KING) check_king_args(opt);
        if (i == PCA) check_pca_args(opt);
        if (i == PVE) check_pve_args(opt);
        if (i == GRM) check_grm_args(opt);
        if (i == LDSCORE) check_ldscore_args(opt);
        if (i == CLUMP) check_clump_args(opt);
        if (i == LDPRUNE) check_ldprune_args(opt);
        if (i == QC) check_qc_args(opt);
        if (i == HOMOZYG) check_homozyg_args(opt);
        if (i == EPISTASIS) (void)epistasis_args(opt); // refuses by name what is out of range
        if (i == CS) check_cs_args(opt);
        if (i == REML) (void)reml_args(opt); // refuses by name what is out of range
    }
}

// every refusal of --sumstats, before anything is read
void check_sumstats(const Options& opt, int nranks)
{
    if (!opt.sumstats) {
        if (const char* o = first_given({{"--sumstats-window", opt.sumstatsWindowGiven}, {"--sumstats-window-kb", opt.sumstatsKbGiven}, {"--sumstats-n", opt.sumstatsNGiven},
                                          {"--sumstats-streams", opt.sumstatsStreamsGiven}, {"--sumstats-chains", opt.sumstatsChainsGiven},
                                          {"--sumstats-post", opt.sumstatsPost}, {"--sumstats-cs", opt.sumstatsCs}}))
            fatal(std::string("FATAL  : ") + o + " needs --sumstats");
    }
    if (!opt.sumstatsCs)
        if (const char* o = first_given({{"--sumstats-cs-r2", !opt.ssCs.r2.empty()}, {"--sumstats-cs-alpha", !opt.ssCs.alpha.empty()}, {"--sumstats-cs-pep", !opt.ssCs.pep.empty()},
                                          {"--sumstats-cs-lead", !opt.ssCs.lead.empty()}, {"--sumstats-cs-max-size", !opt.ssCs.maxSize.empty()},
                                          {"--sumstats-cs-out", !opt.ssCs.out.empty()}}))
            fatal(std::string("FATAL  : ") + o + " needs --sumstats-cs");
    if (!opt.sumstatsPost)
        if (const char* o = first_given({{"--sumstats-post-all", opt.sumstatsPostAll}, {"--sumstats-post-only", opt.sumstatsPostOnly},
                                          {"--sumstats-post-out", !opt.sumstatsPostOut.empty()}}))
            fatal(std::string("FATAL  : ") + o + " needs --sumstats-post");
    if (!opt.sumstats) return;
    if (opt.sumstatsPost) {
        const unsigned T = post_records(opt, opt.sumstatsPostAll);
        if (T < 4)
            fatal("FATAL  : --sumstats-post: T = " + std::to_string(T) + " record(s) per chain (--chain-length " + std::to_string(opt.chainLength) + ", --burn-in " +
                  std::to_string(opt.burnin) + ", --thin " + std::to_string(opt.thin) + (opt.sumstatsPostAll ? ", every iteration at or after the burn-in" : ", the thinned iterations at or after the burn-in") +
                  "): split-R^ of the halved chains needs at least 4");
    }
    if (opt.sumstatsCs) {
        check_cs_values("--sumstats-cs", opt.ssCs);
        check_cs_plan("--sumstats-cs", opt);
    }
    if (opt.bayesType == "bayesWMPI") fatal("FATAL  : --sumstats takes a bayesMPI command line, not --mpibayes bayesWMPI");
    const std::pair<const char*, bool> modes[] = {
        {"--predict-bfile", !opt.predictBfile.empty()}, {"--ld-window", opt.ldGiven}, {"--assoc", opt.assoc}, {"--king", opt.king}, {"--pca", opt.pca}, {"--pve", opt.pve},
        {"--grm", opt.grm}, {"--ld-score", opt.ldScore}, {"--clump", opt.clump}, {"--ld-prune", opt.ldPrune}, {"--he", opt.he}, {"--qc", opt.qc}, {"--homozyg", opt.homozyg},
        {"--epistasis", opt.epistasis}, {"--cs", opt.cs}, {"--reml", opt.reml}};
    for (const auto& m : modes)
        if (m.second) fatal(std::string("FATAL  : --sumstats cannot be combined with ") + m.first + ": it samples a chain, the analysis modes sample nothing");
    if (opt.covariates) fatal("FATAL  : --sumstats cannot be combined with --covariates: summary statistics carry no individual-level covariates");
    if (nranks > 1) fatal("FATAL  : --sumstats runs on one process (WORLD_SIZE = " + std::to_string(nranks) + ")");
    if (const char* o = first_given({{"--restart", opt.restart}, {"--save", opt.saveGiven}, {"--ignore-xfiles", opt.ignoreXfilesGiven}}))
        fatal(std::string("FATAL  : --sumstats cannot be combined with ") + o + ": checkpoint and restart are not built for it");
    if (opt.bedFile.empty())
        fatal("FATAL  : --sumstats needs --bfile: its .fam and .bim name the panel's rows and markers (the genotypes may still come from --sparse-dir/--sparse-basename)");
    if (opt.sumstatsWindowGiven && opt.sumstatsKbGiven) fatal("FATAL  : --sumstats-window-kb cannot be combined with --sumstats-window: one way to define the window");
    long w = 0;
    double t = 0.0;
    if (opt.sumstatsKbGiven && (!whole_num(opt.sumstatsKb, t) || !std::isfinite(t) || t < 0.0))
        fatal("FATAL  : --sumstats-window-kb " + opt.sumstatsKb + ": the window must be a finite number of kilobases >= 0");
    if (opt.sumstatsWindowGiven && (!whole_int(opt.sumstatsWindow, w) || w < 1 || w > 4096))
        fatal("FATAL  : --sumstats-window " + opt.sumstatsWindow + ": the window must be an integer from 1 to 4096 markers (the widest hgibbs_ss_begin takes)");
    if (opt.sumstatsNGiven && (!whole_num(opt.sumstatsN, t) || !std::isfinite(t) || !(t >= 2.0)))
        fatal("FATAL  : --sumstats-n " + opt.sumstatsN + ": the sample size must be a finite number >= 2");
    if (opt.sumstatsStreamsGiven && (!whole_int(opt.sumstatsStreams, w) || w < 1 || w > 1024))
        fatal("FATAL  : --sumstats-streams " + opt.sumstatsStreams + ": the number of streams must be an integer from 1 to 1024 (the most hgibbs_ss_sweep_streams takes)");
    if (opt.sumstatsChainsGiven && (!whole_int(opt.sumstatsChains, w) || w < 1 || w > 64))
        fatal("FATAL  : --sumstats-chains " + opt.sumstatsChains + ": the number of chains must be an integer from 1 to 64 (the most hgibbs_ss_replicas takes)");
}

} // namespace

int main(int argc, const char* argv[])
{
    if (argc < 2) {
        std::cerr << " \nDid you forget to give the input parameters?\n" << std::endl;
        return 1;
    }
    Options opt = parse(argc, argv);
    const char* e;
    const int rank = (e = std::getenv("RANK")) ? std::atoi(e) : 0;
    const int nranks = (e = std::getenv("WORLD_SIZE")) ? std::atoi(e) : 1;
    const int local_rank = (e = std::getenv("LOCAL_RANK")) ? std::atoi(e) : rank;
    if (opt.bedToSparse) return run_bed_to_sparse(opt, nranks, local_rank); // main.cpp:47-55: samples nothing, needs no --mpibayes
    if (!((opt.bayesType == "bayesMPI" || opt.bayesType == "bayesWMPI") && opt.analysisType == "RAM")) {
        std::cerr << "\n Error: Wrong analysis requested: " << opt.analysisType << " + " << opt.bayesType
                  << " (this build reproduces --mpibayes bayesMPI and bayesWMPI)" << std::endl;
        return 0; // the reference catches the throw and still returns 0 (main.cpp:179-189)
    }
    const bool haveBed = !opt.bedFile.empty();
    if (!haveBed && !use_sparse(opt)) fatal("FATAL: either go for BED, SPARSE or BOTH (give --bfile, or --sparse-dir with --sparse-basename)");
    if ((opt.groupIndexFile.empty()) != (opt.groupMixtureFile.empty()))
        fatal("FATAL   : you need to activate both --groupIndexFile and --groupMixtureFile");
    if (opt.syncRate > 1)
        std::printf("WARNING: --sync-rate %d ignored: individuals are sharded, every marker sees the current residual\n", opt.syncRate);

    check_modes(opt, nranks);
    check_sumstats(opt, nranks);
    if (opt.bayesType == "bayesWMPI") return run_bayesw(opt, rank, nranks, local_rank); // main.cpp:164-167

    // ---- inputs (main.cpp:69-70,88; BayesRRm.cpp:969-997) -------------------
    const Dims dims = read_dims(opt); // without --bfile the phenotype file is read line by line
    const size_t numInds = dims.numInds, numSnps = dims.numSnps;
    const std::vector<std::string>& fam_ids = dims.fam_ids;
    std::vector<double> y;
    std::vector<uint8_t> keep;
    std::vector<double> covX;
    int C = 0;
    if (opt.sumstats && opt.phenotypeFile.empty()) { // --pheno only selects the panel's rows there: without it every row is kept
        y.assign(numInds, 0.0);
        keep.assign(numInds, 1);
    } else if (opt.covariates) read_phen_cov(opt.phenotypeFile, opt.covariatesFile, numInds, y, keep, covX, C); // main.cpp:80-83
    else if (haveBed) read_phen(opt.phenotypeFile, fam_ids, y, keep);
    else read_phen_lines(opt.phenotypeFile, numInds, y, keep);
    const unsigned numNAs = (unsigned)(numInds - y.size());

    const unsigned Mtot = check_dims(opt, dims);
    if (Mtot < numSnps && rank == 0) std::printf("INFO   : Option passed to process only %d markers!\n", Mtot);
    const unsigned Ntot = (unsigned)numInds - numNAs;
    if (rank == 0) {
        if (numNAs)
            std::printf("WARNING: opt.numberIndividuals set to %zu but will be adjusted to %zu - %u = %u due to NAs in phenotype file.\n",
                        numInds, numInds, numNAs, Ntot);
        std::printf("INFO   : Full dataset includes Mtot=%d markers and Ntot=%d individuals.\n", Mtot, (int)numInds);
    }
    if (use_sparse(opt)) {
        open_sparse(opt, numInds, Mtot);
        sparse_info(opt, rank, nranks);
    }
    const Cohort co{keep, (unsigned)numInds, numNAs, Ntot, Mtot, local_rank};
    if (!opt.predictBfile.empty()) return run_predict(opt, co);
    if (opt.ldGiven) return run_ld(opt, co);
    if (opt.assoc) return opt.assocLogistic ? run_assoc_logistic(opt, co, y, covX, C) : run_assoc(opt, co, y, covX, C);
    if (opt.king) return run_king(opt, co);
    if (opt.pca) return run_pca(opt, co);
    if (opt.pve) return run_pve(opt, co);
    if (opt.grm) return run_grm(opt, co);
    if (opt.ldScore) return run_ldscore(opt, co);
    if (opt.clump) return run_ldselect(opt, co, true);
    if (opt.ldPrune) return run_ldselect(opt, co, false);
    if (opt.he) return run_he(opt, co, y, covX, C);
    if (opt.qc) return run_qc(opt, co);
    if (opt.homozyg) return run_homozyg(opt, co);
    if (opt.epistasis) return run_epistasis(opt, co, y);
    if (opt.cs) return run_cs(opt, co);
    if (opt.reml) return run_reml(opt, co, y, covX, C);

    const Mixtures mix = read_mixtures(opt, Mtot, true);
    const int G = mix.G, K = mix.K;
    if (opt.sumstats) return run_sumstats(opt, co, mix.groups, mix.mS_flat, G, K);

    adjust_save(opt, rank == 0, false);
    if (rank == 0) make_out_dir(opt);
    // a restart reads <name>.* and writes <name>_rs.* so the failed job's files stay untouched (:1206-1220)
    const std::string base_in = opt.mcmcOutDir + "/" + opt.mcmcOutNam;
    const std::string base = opt.restart ? base_in + "_rs" : base_in;

    // ---- device and genotypes -------------------------------------------------
    hgibbs_t dev = open_device(opt, base, rank, nranks, local_rank, opt.cpg);
    const Shard sh = shard_of(Ntot, rank, nranks);
    load_and_report(dev, opt, numInds, Mtot, numNAs ? keep.data() : nullptr, sh, Ntot, rank);

    hydra_model_desc md{};
    md.seed = opt.seed + (unsigned)0 * 1000; // every rank replicates rank 0's stream (BayesRRm.cpp:1228 with rank = 0)
    md.shuffle = opt.shuffleMarkers;
    md.G = G;
    md.K = K;
    md.groups = mix.groups.empty() ? nullptr : mix.groups.data();
    md.mS = mix.mS_flat.data();
    hydra_chain_t chain = nullptr;
    hg_check(hydra_chain_create(dev, &md, y.data(), &chain), "hydra_chain_create");
    if (opt.covariates) {
        if (rank == 0) std::printf("INFO   : using covariate file: %s\n", opt.covariatesFile.c_str());
        hg_check(hydra_chain_set_covariates(chain, covX.data(), C), "hydra_chain_set_covariates");
    }

    // ---- --restart: BayesRRm::init_from_restart, :842-928, then :1546-1597 -----
    unsigned iteration_start = 0;
    if (opt.restart) {
        if (rank == 0) std::printf("RESTART: from files: %s.* files\n", base_in.c_str());
        const CsvRestart cr = read_csv_for_restart(base_in + ".csv", opt.thin, opt.save, G, K);
        if (rank == 0) {
            std::printf("RESTART: Reading .cvs file %s\n", (base_in + ".csv").c_str());
            std::printf("RESTART: --thin %d  -- save %d\n", opt.thin, opt.save);
            std::printf("RESTART: iteration_to_restart_from = %d\n", cr.iteration_to_restart_from);
            std::printf("RESTART: first_thinned_iteration   = %d\n", cr.first_thinned_iteration);
            std::printf("RESTART: first_saved_iteration     = %d\n", cr.first_saved_iteration);
        }
        if (cr.iteration_to_restart_from == 0)
            fatal("FATAL  : There is no point in restarting a chain from iteration 0 (not saved anyway)\n         => restart your analysis from scratch");
        const unsigned it_from = cr.iteration_to_restart_from;
        RestartState r;
        read_restart_effects(r, opt, base_in, Mtot, it_from, cr.first_thinned_iteration);
        double r_mu = 0.0;
        { // .mus.<rank>: (iteration, mu) per thinned iteration, data.cpp:207-252
            const std::string mp = base_in + ".mus." + std::to_string(rank);
            FILE* f = open_ro(mp);
            const long off = (long)((it_from - cr.first_thinned_iteration) / opt.thin) * (long)(sizeof(unsigned) + sizeof(double));
            unsigned it_ = ~0u;
            pread_at(f, off, &it_, sizeof(unsigned), mp);
            expect_u(it_, it_from, mp + " iteration");
            pread_at(f, off + (long)sizeof(unsigned), &r_mu, sizeof(double), mp);
            std::fclose(f);
        }
        read_restart_shard(r, base_in, rank, it_from, Ntot, sh, Mtot);
        std::vector<uint8_t> gb, xb;
        if (opt.covariates) {
            unsigned len = 0;
            gb = read_dump(base_in + ".gam." + std::to_string(rank), it_from, sizeof(double), &len);
            expect_u(len, (unsigned)C, ".gam length");
            xb = read_dump(base_in + ".xiv." + std::to_string(rank), it_from, sizeof(int32_t), &len);
            expect_u(len, (unsigned)C, ".xiv length");
        }
        hydra_restart_state rs{};
        rs.iteration = it_from;
        rs.sigmaE = cr.sigmaE;
        rs.mu = r_mu;
        rs.sigmaG = cr.sigmaG.data();
        rs.estPi = cr.pi.data();
        rs.beta = r.beta.data();
        rs.components = r.comp.data();
        rs.eps = r.eps;
        rs.order = r.order();
        rs.gamma = opt.covariates ? (const double*)gb.data() : nullptr;
        rs.xI = opt.covariates ? (const int32_t*)xb.data() : nullptr;
        read_rng_file(base_in + ".rng." + std::to_string(rank), &rs.rng);
        hg_check(hydra_chain_restore(chain, &rs), "hydra_chain_restore");
        iteration_start = it_from + 1;
        if (rank == 0) print_restart_banner(base_in, it_from, iteration_start);
    }

    // ---- outputs (rank 0 writes the shared files) ----------------------------
    OutFiles outs;
    FILE *outf = nullptr, *betf = nullptr, *cpnf = nullptr, *acuf = nullptr, *xbetf = nullptr, *xcpnf = nullptr;
    if (rank == 0) {
        outf = outs.open(base + ".csv");
        betf = outs.open(base + ".bet");
        cpnf = outs.open(base + ".cpn");
        acuf = outs.open(base + ".acu");
        xbetf = outs.open(base + ".xbet");
        xcpnf = outs.open(base + ".xcpn");
        for (FILE* f : {betf, xbetf, cpnf, xcpnf, acuf}) pwrite_at(f, 0, &Mtot, sizeof(unsigned)); // :1302-1309
    }
    FILE* musf = outs.open(base + ".mus." + std::to_string(rank));
    FILE* epsf = outs.open(base + ".eps." + std::to_string(rank));
    FILE* mrkf = outs.open(base + ".mrk." + std::to_string(rank));
    FILE* gamf = outs.open(base + ".gam." + std::to_string(rank));
    FILE* xivf = outs.open(base + ".xiv." + std::to_string(rank));
    std::vector<double> gamma(C);
    std::vector<int32_t> xiv(C);

    std::vector<double> beta(Mtot), acum(Mtot), eps(sh.rows());
    std::vector<int32_t> comp(Mtot);
    std::vector<double> sigmaG(G);
    std::vector<int32_t> m0(G);
    std::vector<char> buff(50000);
    unsigned n_thinned_saved = 0;
    const double t_all = now_s();

    for (unsigned iteration = iteration_start; iteration < opt.chainLength; ++iteration) {
        const double t0 = now_s();
        hg_check(hydra_chain_iterate(chain), "hydra_chain_iterate");
        const double t1 = now_s();
        double sigmaE = 0, mu = 0;
        hydra_chain_state(chain, &sigmaE, &mu, sigmaG.data(), nullptr, m0.data(), nullptr, nullptr);
        double sg = 0;
        long m0s = 0;
        for (int g = 0; g < G; ++g) {
            sg += sigmaG[g];
            m0s += m0[g];
        }
        if (rank % 10 == 0) { // :2713-2722 (sync columns are zero: there is no marker-sharded sync in this build)
            std::printf("RESULT : it %4d, rank %4d: proc = %9.3f s, sync = %9.3f (%9.3f + %9.3f), n_sync = %8d (%8d + %8d) (%7.3f / %7.3f), "
                        "sigmaG = %15.10f, sigmaE = %15.10f, betasq = %15.10f, m0 = %10ld\n",
                        iteration, rank, t1 - t0, 0.0, 0.0, 0.0, 0, 0, 0, 0.0, 0.0, sg, sigmaE, 0.0, m0s);
            std::fflush(stdout);
        }

        if (iteration % opt.thin == 0) { // :2736-2794
            hg_check(hgibbs_get_beta(dev, beta.data(), comp.data(), acum.data()), "hgibbs_get_beta");
            if (rank == 0) {
                const int len = hydra_chain_csv_line(chain, iteration, buff.data(), buff.size());
                write_line(outf, n_thinned_saved, buff.data(), len);
                write_thinned(betf, n_thinned_saved, iteration, beta.data(), Mtot, sizeof(double));
                write_thinned(acuf, n_thinned_saved, iteration, acum.data(), Mtot, sizeof(double));
                write_thinned(cpnf, n_thinned_saved, iteration, comp.data(), Mtot, sizeof(int));
            }
            write_mus(musf, n_thinned_saved, iteration, mu);
            n_thinned_saved += 1;
        }

        if (iteration > 0 && iteration % opt.save == 0) { // :2802-2838 (no tarball)
            hgibbs_rng_state rst;
            hydra_chain_state(chain, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &rst);
            write_rng_file(base + ".rng." + std::to_string(rank), rst);
            hg_check(hgibbs_get_residual(dev, eps.data()), "hgibbs_get_residual");
            write_dump(epsf, iteration, sh.rows(), eps.data(), sizeof(double));
            write_dump(mrkf, iteration, Mtot, hydra_chain_order(chain), sizeof(int));
            if (opt.covariates) { // :2810-2832
                hydra_chain_gamma(chain, gamma.data(), xiv.data());
                write_dump(gamf, iteration, (unsigned)C, gamma.data(), sizeof(double));
                write_dump(xivf, iteration, (unsigned)C, xiv.data(), sizeof(int));
            }
            if (rank == 0) {
                hg_check(hgibbs_get_beta(dev, beta.data(), comp.data(), nullptr), "hgibbs_get_beta");
                write_xfile(xbetf, iteration, beta.data(), Mtot, sizeof(double));
                write_xfile(xcpnf, iteration, comp.data(), Mtot, sizeof(int));
            }
        }
    }
    if (rank == 0)
        std::printf("INFO   : rank %4d, time to process the data: %.3f sec, with %.3f (%.3f, %.3f) = %4.1f%% spent on allred (%d, %d)\n", rank,
                    now_s() - t_all, 0.0, 0.0, 0.0, 0.0, 0, 0);
    outs.close(false);
    hydra_chain_destroy(chain);
    hgibbs_destroy(dev);
    return 0;
}
