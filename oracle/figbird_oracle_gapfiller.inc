// figbird_oracle_gapfiller.inc -- TEST INFRASTRUCTURE (textually part of figbird_oracle.cpp).
// Restatement of class GapFiller (Figbird.cpp:1563-6684), the per-gap driver
// (Figbird.cpp:7219-7466) and the FillGaps.cpp merge / scaffold rebuild (FillGaps.cpp:688-926).
// Per-gap read files are parsed once into records; every function then applies the same
// per-function read caps the reference applies while re-reading the file.

struct PartialRec {                 // one line of partial_gaps_<g>.sam (Preprocess.cpp:454)
    string seq; int clipped_index = 0; int match = 0; int pos = 0; int ref_pos = 0;
    string qual;                    // 7th token as strtok("\t") yields it (may end in '\n')
};

// Globals of Figbird.cpp that GapFiller reads/writes (Figbird.cpp:99-147).
int left_maxDistance, right_maxDistance;
int factor_g, covergae_threshold1, covergae_threshold2, partial_threshold, overlap_threshold;
int match_count_discont, clip_thresh, num_itr, alloc_arg, step2match;
vector<int> gaptofill;
FILE *drawf = nullptr;

static string safe_substr(const string &s, long pos, long n) {
    if (pos < 0 || (size_t)pos > s.size()) {
        fprintf(stderr, "oracle: substr out of range (reference would throw std::out_of_range)\n");
        abort();
    }
    if (n < 0) n = (long)string::npos;      // size_t wrap => "to the end"
    return s.substr((size_t)pos, (size_t)n);
}

struct GF {
    typedef double Row[5];
    vector<double> countsGap_, new_counts_gap_, probsGap_, errorProbsGap_, qual_gap_, partial_count_array_;
    double *countsGap(long i) { return &countsGap_[i * 5]; }
    double *new_counts_gap(long i) { return &new_counts_gap_[i * 5]; }
    double *probsGap(long i) { return &probsGap_[i * 5]; }
    double *errorProbsGap(long i) { return &errorProbsGap_[i * 5]; }
    double *qual_gap(long i) { return &qual_gap_[i * 5]; }
    double *partial_count_array(long i) { return &partial_count_array_[i * 5]; }
    vector<int> gap_coverage;
    vector<vector<double>> partial_read_quality;

    int gap_no = 0, contigNo = 0; long gapStart = 0; int gapLength = 0;
    int valid_count = 0, invalid_count = 0, partial_read_count = 0, p_count = 0;
    double region_perct = 0, region_perct_max_gap_estm = 0; long end_pos_max = 0;
    int originalGap = 0, partial_read_len = 0, unmapped_read_len = 0, max_read_len = 0;
    int fillNotfill = 0, perfectReadGap = 0, perfectReadGaplen = 0;
    vector<int> repeatflag;         // [p][3]
    int rep_flag = 0, one_side_repeat_flag = 0, large_gap_flag = 0, part_read_c = 0;
    int fill_original = 0, comp_count = 0;
    long startPos = 0, endPos = 0;
    string concensus, bestString, secondBestString, current_str, previous_str;
    vector<string> reads_gap; vector<int> pos_reads, isReverse;
    int num_reads_in_gap = 0;
    vector<int> mark_accepted_reads; vector<double> maxlikelihood_value;
    vector<int> final_readpos;      // [r][3]
    vector<int> saved_reads;
    int maxGap = 0, left_max = 0, right_min = 0, discont_or_not = 0;
    string gap_left, gap_right, partial_left, partial_right;
    int partial_saved_read_temp[2], partial_saved_read_final[2];
    int side_limit = 30;
    vector<int> unmapped_read_pos_arr_org, partial_read_pos_arr_org;   // [r][3]
    long maxSize = 0; int mid_limitu = 0, mid_limitp = 0; float gp_frac1 = 0, gp_frac2 = 0;
    int umaxleftf = 0, umaxrightf = 0, ucoverf = 0, negoverlap = 0;

    const string *contig = nullptr; long contigLen = 0;
    vector<PartialRec> *prec = nullptr;     // all lines of the partial file
    vector<string> *ulines = nullptr;       // all lines of the gaps file

    // ------------------------------------------------------------------ allocate :1638-1778
    void allocate(int maxGap_, int read_count, int read_count2, int len, int stat1, int stat2, int stat3,
                  int neglap, int mp, int up, int lgf, float gpf1, float gpf2) {
        maxGap = maxGap_; negoverlap = neglap; mid_limitu = up; mid_limitp = mp;
        gp_frac1 = gpf1; gp_frac2 = gpf2; large_gap_flag = lgf;
        num_reads_in_gap = read_count; partial_read_count = read_count2;
        side_limit = 30;
        maxSize = (long)maxGap + 2L * A.D;
        concensus.assign(1, 'N'); concensus.clear(); concensus = "N";
        end_pos_max = 0; valid_count = invalid_count = 0; p_count = 0;
        countsGap_.assign(maxSize * 5, 0.0); probsGap_.assign(maxSize * 5, 0.0);
        errorProbsGap_.assign(maxSize * 5, 0.0); new_counts_gap_.assign(maxSize * 5, 0.0);
        qual_gap_.assign((size_t)maxGap * 5, 0.0); gap_coverage.assign(maxGap, 0);
        partial_count_array_.assign((size_t)maxGap * 5, 0.0);
        unmapped_read_len = len; partial_read_len = mp / 2;
        fillNotfill = stat1; perfectReadGap = stat2; perfectReadGaplen = stat3;
        rep_flag = 0; one_side_repeat_flag = 0; fill_original = 0; region_perct = 0; part_read_c = 0;
        if (read_count > 0) {
            pos_reads.assign(read_count, 0); isReverse.assign(read_count, 0);
            mark_accepted_reads.assign(read_count, 0); saved_reads.assign(read_count, 0);
            reads_gap.assign(read_count, string());
            unmapped_read_pos_arr_org.assign((size_t)read_count * 3, 0);
            final_readpos.assign((size_t)read_count * 3, 0);
            for (int i = 0; i < read_count; i++) {
                unmapped_read_pos_arr_org[i * 3] = -200;
                final_readpos[i * 3] = -200; final_readpos[i * 3 + 1] = 0; final_readpos[i * 3 + 2] = -1;
            }
        }
        maxlikelihood_value.assign(std::max(std::max(read_count, read_count2), 1), 0.0);
        if (partial_read_count > 0) {
            partial_read_pos_arr_org.assign((size_t)partial_read_count * 3, 0);
            for (int i = 0; i < partial_read_count; i++) partial_read_pos_arr_org[i * 3 + 1] = -200;
        }
        bestString.clear(); secondBestString.clear(); current_str.clear(); previous_str.clear();
        gap_left.clear(); gap_right.clear();
        for (int i = 0; i < 2; i++) partial_saved_read_temp[i] = partial_saved_read_final[i] = -1;
    }

    char ctg(long i) const {                    // contigs[contigNo][i]; out-of-range is UB in the reference
        if (i < 0 || i >= contigLen) return '\0';
        return (*contig)[i];
    }

    // ------------------------------------------------------------------ findRepeat :1799-1911
    int findRepeat() {
        int flag1 = 0, flag2 = 0, flag = 0;
        int pc = 0;
        for (size_t k = 0; k < prec->size(); k++) { pc++; if (pc > partial_limit) break; }
        part_read_c = pc;
        if (pc > 0) {
            repeatflag.assign((size_t)pc * 3, -1);
            pc = 0;
            vector<size_t> positions;
            for (size_t k = 0; k < prec->size(); k++) {
                const string &s5 = (*prec)[k].seq;
                int n = 20;
                const string &s1 = gap_left, &s2 = gap_right;
                int lim = (int)gap_left.size() - n;
                for (int i = 0; i < lim; i++) {
                    string s3 = s1.substr(i);
                    size_t pos = s5.find(s3, 0);
                    while (pos != string::npos) { positions.push_back(pos); pos = s5.find(s3, pos + 1); }
                    if (positions.size() > 1) {
                        repeatflag[pc * 3 + 0] = 1; repeatflag[pc * 3 + 1] = (int)s3.length();
                        repeatflag[pc * 3 + 2] = (int)positions[0];
                        flag1 = 1; flag2 = pc; one_side_repeat_flag = 1;
                        break;
                    }
                    positions.clear();
                }
                positions.clear();
                lim = (int)gap_right.size() - n;
                for (int i = 0; i < lim; i++) {
                    string s4 = s2.substr(0, s2.size() - i);
                    size_t pos = s5.find(s4, 0);
                    while (pos != string::npos) { positions.push_back(pos); pos = s5.find(s4, pos + 1); }
                    if (positions.size() > 1) {
                        repeatflag[pc * 3 + 0] = 2; repeatflag[pc * 3 + 1] = (int)positions[positions.size() - 1];
                        if (flag1 == 1 && pc == flag2) flag = 1;
                        one_side_repeat_flag = 1;
                        break;
                    }
                    positions.clear();
                }
                positions.clear();
                pc++;
                if (pc > partial_limit) break;
            }
        }
        return flag;
    }

    // ------------------------------------------------------------------ update_partial_prob :1913-2088
    void update_partial_prob(int gaplen) {
        int val = MAX_GAP;
        left_max = -val; right_min = val;
        for (int i = 0; i < gaplen; i++) for (int j = 0; j <= 4; j++) partial_count_array(i)[j] = 1;
        int pc = 0;
        for (size_t k = 0; k < prec->size(); k++) {
            const PartialRec &r = (*prec)[k];
            const string &rs = r.seq;
            int clipped_index = r.clipped_index, match = r.match, len = (int)rs.size();
            if (len > partial_read_len) partial_read_len = len;
            if (repeatflag[pc * 3] != -1) {
                if (repeatflag[pc * 3] == 1) clipped_index = repeatflag[pc * 3 + 2] + repeatflag[pc * 3 + 1] - 1;
                if (repeatflag[pc * 3] == 2) clipped_index = repeatflag[pc * 3 + 1];
            }
            int stop_index1 = std::min(len - clipped_index - 1, gaplen);
            int stop_index2 = (clipped_index <= gaplen) ? 0 : clipped_index - gaplen;
            if (match == 1 || match == 4) {
                int j = 0;
                for (int i = clipped_index + 1; i < clipped_index + 1 + stop_index1; i++, j++) {
                    int c = cc(rs[i]);
                    if (c < 4) partial_count_array(j)[c] += 1;
                    else for (int h = 0; h < 4; h++) partial_count_array(j)[h] += 1;
                }
                if (j - 1 > left_max) left_max = j - 1;
            } else if (match == 2 || match == 3) {
                int j = gaplen - 1;
                for (int i = clipped_index - 1; i >= stop_index2; i--, j--) {
                    int c = cc(rs[i]);
                    if (c < 4) partial_count_array(j)[c] += 1;
                    else for (int h = 0; h < 4; h++) partial_count_array(j)[h] += 1;
                }
                if (j + 1 < right_min) right_min = j + 1;
            }
            pc++;
            if (pc > partial_limit) break;
        }
        if (A.partial_flag == 1) partial_read_count = pc;
        int total_count_p = 0, left_c = 0, right_c = 0;
        char pl[100], pr[100];
        for (int i = 0; i < gaplen; i++) {
            total_count_p = 0;
            int max_index = 0, max_val = -1;
            for (int k = 0; k < 4; k++) {
                total_count_p += partial_count_array(i)[k];
                if (partial_count_array(i)[k] > max_val) { max_val = (int)partial_count_array(i)[k]; max_index = k; }
            }
            if (i <= left_max - 5 || i >= right_min + 5) {
                char ch = max_index == 0 ? 'A' : max_index == 1 ? 'C' : max_index == 2 ? 'G' : 'T';
                // partial_left/right are char[100] in the reference (:1625); >99 majority chars overflow there.
                if (i <= left_max - 5) { if (left_c < 99) pl[left_c++] = ch; }
                else { if (right_c < 99) pr[right_c++] = ch; }
            }
            for (int k = 0; k < 4; k++)
                probsGap(i + left_maxDistance)[k] = partial_count_array(i)[k] / total_count_p;
        }
        pl[left_c] = '\0'; pr[right_c] = '\0';
        partial_left = pl; partial_right = pr;
    }

    // ------------------------------------------------------------------ computeProbsGap :2090-2116
    void computeProbsGap(int flag) {
        for (long i = 0; i < endPos - startPos; i++) {
            double total = 0;
            for (int j = 0; j < 5; j++) total = total + countsGap(i)[j];
            double Ncount = countsGap(i)[4];
            for (int j = 0; j < 4; j++) {
                if (total) probsGap(i)[j] = ((countsGap(i)[j] + (Ncount / 4)) / total);
                else probsGap(i)[j] = .25;
            }
            probsGap(i)[4] = 0;
        }
        if (flag == 1) update_partial_prob(gapLength);
    }

    // ------------------------------------------------------------------ computeErrorProbsGap :2118-2137
    void computeErrorProbsGap() {
        for (long i = 0; i < endPos - startPos; i++)
            for (int j = 0; j < 5; j++) {
                double sum = 0;
                for (int k = 0; k < 4; k++) { if (j == k) continue; sum += probsGap(i)[k] * (M.errorTypeProbs[k][j]); }
                errorProbsGap(i)[j] = sum;
            }
    }

    // ------------------------------------------------------------------ initialize_start_end :2269-2296
    void initialize_start_end() {
        if (gapStart - left_maxDistance < 0) {
            startPos = 0;
            left_maxDistance = (int)gapStart;
            if (side_limit > left_maxDistance) side_limit = left_maxDistance;
        } else startPos = gapStart - left_maxDistance;
        if (gapStart + gapLength + right_maxDistance > contigLen) {
            endPos = contigLen;
            right_maxDistance = (int)(contigLen - (gapStart + gapLength));
            if (side_limit > right_maxDistance) side_limit = right_maxDistance;
        } else endPos = gapStart + gapLength + right_maxDistance;
        if (endPos > end_pos_max) end_pos_max = endPos;
    }

    // ------------------------------------------------------------------ findGapLeftRight :2151-2174
    void findGapLeftRight() {
        gapLength = originalGap;
        initialize_start_end();
        gap_left.clear(); gap_right.clear();
        for (long i = 0; i < left_maxDistance; i++)
            if (left_maxDistance - i <= side_limit) gap_left.push_back(ctg(i + startPos));
        int c_j = 0;
        for (long i = left_maxDistance + gapLength; i < left_maxDistance + gapLength + right_maxDistance; i++)
            if (c_j < side_limit) { gap_right.push_back(ctg(i + startPos - gapLength + originalGap)); c_j++; }
    }

    // ------------------------------------------------------------------ find_contig_match :2176-2267
    int find_contig_match() {
        if (originalGap > negoverlap) return 0;
        int n = 3;
        const string &s1 = gap_left, &s2 = gap_right;
        for (int i = 0; i < side_limit - n; i++) {
            if ((size_t)i > s1.size() || (size_t)i > s2.size()) break;   // substr would throw / size_t wrap
            string s3 = s1.substr(i);
            string s4 = s2.substr(0, s2.size() - i);
            int pos = (int)s3.find(s4);
            if (pos != -1) {
                string rem_str = s2.substr(s4.size());
                int error_thresh = 2, part_count = 0;
                for (size_t k = 0; k < prec->size(); k++) {
                    const string &rs = (*prec)[k].seq;
                    int len = (int)rs.size(), max_match = -1, max_pos = -1;
                    // `j<len-s1.size()` is an unsigned comparison in the reference (:2209)
                    for (size_t j = 0; j < (size_t)len - s1.size(); j++) {
                        if ((size_t)len < s1.size()) break;              // wrapped bound: reference reads out of bounds
                        int match_count = 0, mismatch = 0;
                        for (size_t kk = 0; kk < s1.size(); kk++) {
                            if (rs[j + kk] == s1[kk]) match_count++; else mismatch++;
                            if (mismatch > error_thresh) break;
                        }
                        if (match_count > max_match) { max_match = match_count; max_pos = (int)j; }
                    }
                    if (s1.size() - max_match <= (size_t)error_thresh) {
                        int newpos = max_pos + (int)s1.size(), match = 0;
                        int matchval = (int)s4.size();
                        for (size_t j = 0; j < rem_str.size(); j++) {
                            char rc = ((size_t)(newpos + j) < rs.size()) ? rs[newpos + j] : '\0';
                            if (rem_str[j] == rc) match++;
                        }
                        if (rem_str.size() - match <= (size_t)error_thresh) return matchval;
                    }
                    part_count++;
                    if (part_count > partial_limit) break;
                }
            }
        }
        return 0;
    }

    // ------------------------------------------------------------------ initialize :2298-2383
    int initialize(int gl, int flag, int negGapCheck) {
        gapLength = gl;
        initialize_start_end();
        for (long i = 0; i < endPos - startPos; i++)
            for (int j = 0; j < 5; j++) { countsGap(i)[j] = 0; probsGap(i)[j] = 0; errorProbsGap(i)[j] = 0; new_counts_gap(i)[j] = 0; }
        region_perct = 0;
        for (size_t i = 0; i < maxlikelihood_value.size(); i++) maxlikelihood_value[i] = 0;
        for (int i = 0; i < maxGap; i++) { for (int j = 0; j < 5; j++) qual_gap(i)[j] = 0; gap_coverage[i] = 0; }
        for (long i = 0; i < left_maxDistance; i++) countsGap(i)[cc(ctg(i + startPos))]++;
        for (long i = left_maxDistance; i < left_maxDistance + gapLength; i++) countsGap(i)[4]++;
        for (long i = left_maxDistance + gapLength; i < left_maxDistance + gapLength + right_maxDistance; i++)
            countsGap(i)[cc(ctg(i + startPos - gapLength + originalGap))]++;
        int gfp = 0;
        if (side_limit > 0 && negGapCheck == 0 && flag == 1) gfp = find_contig_match();
        computeProbsGap(flag);
        computeErrorProbsGap();
        return gfp;
    }

    // ------------------------------------------------------------------ draw_read :2385-2427
    void draw_read(int length, const char *s, int readno, int isz, int g, char type) {
        if (!drawf) return;
        int readlen = unmapped_read_len;
        if (s[0] == 'S') {
            for (int i = 0; i < readlen; i++) fputc(' ', drawf);
            fprintf(drawf, "====================+Gap = %d starting,length = %d===============================\n", g, length);
            for (int i = 0; i < readlen; i++) fputc(' ', drawf);
            for (int i = 0; i < length; i++) fputc('N', drawf);
            fputc('\n', drawf);
        } else {
            for (int i = 0; i < readlen + length; i++) fputc(' ', drawf);
            fprintf(drawf, "%s[", s);
            fprintf(drawf, "%d %d isz = %d %c]", readno, length, isz, type);
            fprintf(drawf, "\n");
        }
    }

    // ------------------------------------------------------------------ getDiff :2429-2443
    static double getDiff(const string &target, const string &ref, int length) {
        double diff = 0;
        for (int i = 0; i < length; i++) if (toupper((unsigned char)target[i]) != ref[i]) diff++;
        return diff / length;
    }

    // ------------------------------------------------------------------ find_partial_match :2445-2490
    int find_partial_match(const string &ref, const string &search, int pos, int c, int len_t) {
        int len_r = (int)ref.size(), len_s = (int)search.size();
        int len_thresh = (c == 0) ? len_t : 4;
        if (len_r >= len_s && len_s >= len_thresh) {
            string s3, s4;
            if (pos == 0) { s3 = ref.substr(ref.size() - len_s, len_s); s4 = search.substr(search.size() - len_s, len_s); }
            else { s3 = ref.substr(0, len_s); s4 = search.substr(0, len_s); }
            double frac = getDiff(s3, s4, len_s);
            if (frac < 0.2 && c == 1) return 1;
            if (frac <= 0.08 && c == 0) return 1;
        }
        return 0;
    }

    // ------------------------------------------------------------------ get_read_frag :2492-2511
    string get_read_frag(const string &s1, int placed_pos) {
        int neg = -placed_pos;
        if (placed_pos < 0) {
            if (neg < side_limit) return safe_substr(s1, 0, neg);
            return safe_substr(s1, neg - side_limit, side_limit);
        }
        return safe_substr(s1, gapLength - placed_pos, side_limit);
    }

    // ------------------------------------------------------------------ detect_overlap_gapestimate :2513-2779
    // pflag: [k*stride + 0] = used flag, [k*stride + 1] = placed position.
    void detect_overlap_gapestimate(const int *pflag, int stride, int gaplen, int *ret_v, int len_thresh) {
        int l_max = -MAX_GAP, r_min = MAX_GAP;
        g_det_nmax = 0; g_det_false = 0;                 // trace only
        vector<int> left_cross, right_cross;
        int pc = 0, overlap_count = 0;
        double mismatch_threshold = .1;
        vector<string> partial_reads(partial_read_count);
        vector<int> match_reads(partial_read_count, 0), sm_flag(partial_read_count, 0);
        for (size_t k = 0; k < prec->size(); k++) {
            if (pc >= partial_read_count) break;            // reference would index past its VLAs
            const PartialRec &r = (*prec)[k];
            int match = r.match, len = (int)r.seq.size();
            match_reads[pc] = match;
            partial_reads[pc] = r.seq;
            if (pflag[pc * stride] == 0) { pc++; if (pc > partial_limit) break; continue; }
            int pos = pflag[pc * stride + 1];
            int j, flag = 0, start = -1;
            for (j = 0; j < len; j++) {
                if (pos + j >= 0 && pos + j < gaplen) { if (flag == 0) { flag = 1; start = pos + j; } }
                if (pos + j == gaplen) break;
            }
            if (match == 1 || match == 4 || pos < 0) { if (pos + j - 1 > l_max) l_max = pos + j - 1; }
            else { if (start < r_min) r_min = start; }
            pc++;
            if (pc > partial_limit) break;
        }
        if (l_max == -MAX_GAP) l_max = -1;
        if (r_min == MAX_GAP) r_min = gaplen;
        overlap_count = l_max - r_min + 1;
        int ovflag = 0;
        for (int k = 0; k < partial_read_count; k++) {
            if (pflag[k * stride] == 1) {
                const string &s1 = partial_reads[k];
                int len = (int)s1.size();
                int placed_pos = pflag[k * stride + 1];
                if (placed_pos < 0 && placed_pos + len > gapLength) {
                    string l = (-placed_pos < side_limit) ? safe_substr(s1, 0, -placed_pos)
                                                          : safe_substr(s1, -placed_pos - side_limit, side_limit);
                    string r = safe_substr(s1, -placed_pos + gapLength, side_limit);
                    if (find_partial_match(gap_left, l, 0, 0, len_thresh) && find_partial_match(gap_right, r, 1, 0, len_thresh))
                        ovflag = 1;
                }
                if (placed_pos < 0 && placed_pos + len - 1 >= r_min && placed_pos + len <= gapLength) left_cross.push_back(k);
                if (placed_pos > 0 && placed_pos <= l_max) right_cross.push_back(k);
                if (placed_pos < 0 && placed_pos + len > gapLength && (match_reads[k] == 2 || match_reads[k] == 3)) {
                    right_cross.push_back(k);
                    sm_flag[k] = 1;
                }
            }
        }
        if (ovflag || (perfectReadGap == 1 && originalGap <= 20 && gaplen == perfectReadGaplen)) {
            ret_v[0] = 300; ret_v[1] = 0;
            return;
        }
        if (r_min <= l_max) {
            int max_overlap = 0, false_overlap_flag = 0;
            for (size_t i = 0; i < left_cross.size(); i++)
                for (size_t j = 0; j < right_cross.size(); j++) {
                    if (left_cross[i] == right_cross[j]) continue;
                    const string &rs1 = partial_reads[left_cross[i]];
                    int p1 = pflag[left_cross[i] * stride + 1];
                    int len = (int)rs1.size();
                    const string &rs2 = partial_reads[right_cross[j]];
                    int p2 = pflag[right_cross[j] * stride + 1];
                    int diff_gap = p1 + len - gaplen;
                    if (diff_gap > 0) overlap_count = (p1 + len - 1) - p2 + 1 - diff_gap;
                    else { overlap_count = (p1 + len - 1) - p2 + 1; diff_gap = 0; }
                    if (overlap_count >= overlap_threshold) {
                        string common_left, common_right;
                        if (sm_flag[right_cross[j]] != 1) {
                            if (find_partial_match(gap_left, get_read_frag(rs1, p1), 0, 1, -1))
                                common_left = safe_substr(rs1, (long)rs1.size() - overlap_count - diff_gap, overlap_count);
                            if (find_partial_match(gap_right, get_read_frag(rs2, p2), 1, 1, -1))
                                common_right = safe_substr(rs2, 0, overlap_count);
                        } else {
                            int x = pflag[right_cross[j] * stride + 1];
                            if (find_partial_match(gap_left, get_read_frag(rs1, p1), 0, 1, -1))
                                common_left = safe_substr(rs1, (long)rs1.size() - overlap_count - x, overlap_count - x);
                            string s3 = safe_substr(rs2, -x + gapLength, side_limit);
                            if (find_partial_match(gap_right, s3, 1, 1, -1))
                                common_right = safe_substr(rs2, -x, overlap_count + x);
                        }
                        int len1 = (int)common_left.size(), len2 = (int)common_right.size();
                        if (len1 > 0 && len2 > 0 && len1 == len2) {
                            double mismatch_frac = getDiff(common_left, common_right, len1);
                            if (mismatch_frac <= mismatch_threshold) {
                                if (len1 == max_overlap) g_det_nmax++;      // trace only
                                if (len1 > max_overlap) {
                                    g_det_nmax = 1;
                                    max_overlap = len1;
                                    partial_saved_read_temp[0] = left_cross[i];
                                    partial_saved_read_temp[1] = right_cross[j];
                                }
                            } else false_overlap_flag = -1;
                        }
                    }
                }
            g_det_false = false_overlap_flag;
            if ((false_overlap_flag == 0 && max_overlap >= overlap_threshold) ||
                (false_overlap_flag == -1 && max_overlap >= 2 * overlap_threshold)) {
                ret_v[0] = max_overlap; ret_v[1] = 0;
            } else if (false_overlap_flag == -1 || max_overlap < overlap_threshold) {
                ret_v[0] = 0; ret_v[1] = -1;
                partial_saved_read_temp[0] = partial_saved_read_temp[1] = -1;
            }
            return;
        }
        ret_v[0] = 0; ret_v[1] = 0;
    }

    struct Trip { int v[3]; };
    static bool sortcol(const Trip &a, const Trip &b) { return a.v[0] < b.v[0]; }

    // ------------------------------------------------------------------ findOverlapUnmapped :2945-3019
    double findOverlapUnmapped(vector<int> &pos) {
        int correct_overlap = 0, incorrect_penalty = 0, gap_penalty = 0, diff = 0;
        vector<Trip> vec(num_reads_in_gap);
        for (int i = 0; i < num_reads_in_gap; i++) for (int j = 0; j < 3; j++) vec[i].v[j] = pos[i * 3 + j];
        std::sort(vec.begin(), vec.end(), sortcol);         // libstdc++ introsort, as the reference binary
        for (int i = 0; i < num_reads_in_gap - 1; i++) {
            if (vec[i].v[0] != -200) {
                diff = (vec[i].v[0] + vec[i].v[1] - vec[i + 1].v[0]);
                if (diff >= match_count_discont) {
                } else if (diff >= 0) {
                    incorrect_penalty += -250;
                    discont_or_not = 1;
                } else {
                    gap_penalty += -4 * 50;
                    mark_accepted_reads[vec[i].v[2]] = 0;
                    mark_accepted_reads[vec[i + 1].v[2]] = 0;
                    if (gapLength == originalGap) {
                        unmapped_read_pos_arr_org[vec[i].v[2] * 3] = -200;
                        unmapped_read_pos_arr_org[vec[i + 1].v[2] * 3] = -200;
                        unmapped_read_pos_arr_org[vec[i].v[2] * 3 + 1] = 0;
                        unmapped_read_pos_arr_org[vec[i + 1].v[2] * 3 + 1] = 0;
                    }
                    valid_count -= 2;
                }
            }
        }
        int left_right_match_count = 0;
        for (int i = 0; i < num_reads_in_gap; i++) {
            if (vec[i].v[0] != -200) {
                if (vec[i].v[0] < 0 && -vec[i].v[0] >= 3 && vec[i].v[0] + vec[i].v[1] > 0) left_right_match_count++;
                if (vec[i].v[0] < gapLength && vec[i].v[0] + vec[i].v[1] - gapLength >= 3) left_right_match_count++;
            }
        }
        int left_right_match_adv = left_right_match_count * 50;
        return (double)(correct_overlap + incorrect_penalty + gap_penalty + left_right_match_adv);
    }

    // gapString of placeReads / finalize (:3304-3323): flanks from the contig, middle from `mid`.
    // Index relative to the window start; out-of-window indices are UB in the reference and
    // read as '\0' (charCode 4) here.
    struct GapString {
        string s;
        char at(long idx) const { return (idx < 0 || idx >= (long)s.size()) ? '\0' : s[idx]; }
    };
    GapString make_gap_string(const string &mid, int gl) {
        GapString g;
        long maxS = gl + (left_maxDistance + right_maxDistance);
        g.s.resize(maxS);
        for (long i = 0; i < left_maxDistance; i++) g.s[i] = ctg(i + startPos);
        for (long i = left_maxDistance; i < left_maxDistance + gl; i++)
            g.s[i] = ((size_t)(i - left_maxDistance) < mid.size()) ? mid[i - left_maxDistance] : '\0';
        for (long i = left_maxDistance + gl; i < left_maxDistance + gl + right_maxDistance; i++)
            g.s[i] = ctg(i + startPos - gl + originalGap);
        return g;
    }

    // E-step factor product for one placement (Figbird.cpp:3142-3167 / 3563-3589).
    inline double estep_product(double tempProb, const string &rs, int j0, int j1, long i, int isRev) {
        int L = (int)rs.size();
        long nrows = maxSize;
        for (int j = j0; j < j1; j++) {
            int charCode = cc(rs[j]);
            long index = i + j - startPos;
            int readIndex = isRev == 1 ? L - 1 - j : j;
            if (index < 0 || readIndex < 0) continue;
            if (index >= nrows) { tempProb *= 0.0; continue; }        // UB in the reference (unallocated row)
            if (charCode < 4)
                tempProb *= (probsGap(index)[charCode] * (1 - M.errorPosDist[readIndex]) +
                             M.errorPosDist[readIndex] * errorProbsGap(index)[charCode]);
            else
                tempProb *= (M.errorPosDist[readIndex] * errorProbsGap(index)[4]);
        }
        g_flops += 4.0 * (j1 - j0);
        return tempProb;
    }
    // MLE product (Figbird.cpp:3383-3407 / 3761-3785).
    inline double mle_product(const string &rs, int j0, int j1, long i, const GapString &gs, int strandRev) {
        double tempProb = 1;
        int L = (int)rs.size();
        for (int j = j0; j < j1; j++) {
            int toCharCode = cc(rs[j]);
            long index = i + j - startPos;
            int fromCharCode = cc(gs.at(index));
            int k = strandRev == 0 ? j : L - j - 1;
            if (fromCharCode == toCharCode) tempProb *= (1 - M.errorPosDist[k] - M.inPosDist[k] - M.delPosDist[k]);
            else if (fromCharCode >= 0 && fromCharCode <= 4) tempProb *= M.errorPosDist[k] * M.errorTypeProbs[fromCharCode][toCharCode];
        }
        g_flops += 1.0 * (j1 - j0);
        return tempProb;
    }

    // ------------------------------------------------------------------ placeReads :3022-4387
    double placeReads(int ge, int g, int finalize_flag, int gapoffset, int updateflag) {
        g_place_calls++;
        double maxProb = 0, tempProb, maxLikelihood = 0, antilog_value = 0;
        int insertSize, tempInsertSize, maxPos;
        for (long i = left_maxDistance; i < endPos - startPos - right_maxDistance; i++)
            for (int j = 0; j < 5; j++) countsGap(i)[j] = 0;
        int count_of_read = num_reads_in_gap;
        for (int i = 0; i < count_of_read; i++) {
            maxlikelihood_value[i] = 0; mark_accepted_reads[i] = 0;
            final_readpos[i * 3] = -200; final_readpos[i * 3 + 1] = 0; final_readpos[i * 3 + 2] = -1;
            if (gapLength == originalGap) {
                unmapped_read_pos_arr_org[i * 3] = -200; unmapped_read_pos_arr_org[i * 3 + 1] = 0; unmapped_read_pos_arr_org[i * 3 + 2] = 0;
            }
        }
        for (int i = 0; i < partial_read_count; i++) maxlikelihood_value[i] = 0;

        if (A.partial_flag) {
            count_of_read = 0;
            vector<double> tr_rmax;              // per-read E-step maxima, kept for the level-3 trace only
            for (size_t k = 0; k < prec->size(); k++) {
                const PartialRec &r = (*prec)[k];
                const string &rs = r.seq;
                int readLength1 = (int)rs.size();
                int flag1 = r.match, pos1 = r.pos, ref_pos = r.ref_pos;
                int isRev = 0, read_start, read_end;
                maxProb = -DBL_MAX; maxPos = 0;
                if (flag1 == 1 || flag1 == 4) { read_start = clip_thresh; read_end = 0; }
                else { read_start = 0; read_end = clip_thresh; }
                count_of_read++;
                if (count_of_read > partial_limit) break;
                if (pos1 < gapStart) {
                    insertSize = (int)(gapStart - ref_pos + readLength1);
                    for (long i = gapStart - readLength1 + 1; i < gapStart; i++) {
                        tempInsertSize = (int)(insertSize + i - gapStart);
                        if ((tempInsertSize < M.insertThresholdMin || tempInsertSize > M.insertThresholdMax) && ref_pos != -1) continue;
                        tempProb = estep_product(1, rs, read_start, readLength1 - read_end, i, isRev);
                        tempProb = LM_LOG(tempProb);
                        if (tempProb > maxProb) { maxProb = tempProb; maxPos = (int)(i - startPos); }
                        antilog_value = LM_POW10(tempProb);
                        for (int j = 0; j < readLength1; j++)
                            if (i - startPos + j >= left_maxDistance && i - startPos + j < left_maxDistance + gapLength)
                                { countsGap(i - startPos + j)[cc(rs[j])] += antilog_value; g_flops += 1.0; }
                    }
                } else {
                    if (ref_pos != -1) ref_pos += gapoffset;
                    insertSize = (int)(ref_pos - (gapStart + gapLength) + readLength1);
                    for (long i = gapStart + gapLength - readLength1 + 1; i < gapStart + gapLength; i++) {
                        tempInsertSize = (int)(insertSize + gapStart + gapLength - i);
                        if ((tempInsertSize < M.insertThresholdMin || tempInsertSize > M.insertThresholdMax) && ref_pos != -1) continue;
                        tempProb = estep_product(1, rs, read_start, readLength1 - read_end, i, isRev);
                        tempProb = LM_LOG(tempProb);
                        if (tempProb > maxProb) { maxProb = tempProb; maxPos = (int)(i - startPos); }
                        antilog_value = LM_POW10(tempProb);
                        for (int j = 0; j < readLength1; j++)
                            if (i - startPos + j >= left_maxDistance && i - startPos + j < left_maxDistance + gapLength)
                                { countsGap(i - startPos + j)[cc(rs[j])] += antilog_value; g_flops += 1.0; }
                    }
                }
                if (maxProb != -DBL_MAX) maxLikelihood += (maxProb);
                if (g_trace && g_trace_level >= 3) tr_rmax.push_back(maxProb != -DBL_MAX ? maxProb : 0.0);   // trace only
            }
            if (g_trace && g_trace_level >= 3) {      // numeric planes (i)/(ii) after the E-step, as in the unmapped branch below
                FILE *tf = trace_plane_file();
                fprintf(tf, "E\t%d\t%d\t%d", g, gapLength, ge);
                for (long i = left_maxDistance; i < left_maxDistance + gapLength; i++)
                    for (int j = 0; j < 5; j++) fprintf(tf, "\t%a", countsGap(i)[j]);
                fprintf(tf, "\nR\t%d\t%d\t%d", g, gapLength, ge);
                for (double v : tr_rmax) fprintf(tf, "\t%a", v);
                fprintf(tf, "\n");
            }
            // ---- MLE pass over partial reads (:3267-3523)
            vector<int> pflag((size_t)partial_read_count * 2);
            for (int i = 0; i < partial_read_count; i++) {
                pflag[i * 2] = 1; pflag[i * 2 + 1] = 0;
                if (gapLength == originalGap) {
                    partial_read_pos_arr_org[i * 3] = 0; partial_read_pos_arr_org[i * 3 + 1] = -200; partial_read_pos_arr_org[i * 3 + 2] = 0;
                }
            }
            computeSequence(0, 0);
            string new_bestString = concensus;
            for (long i = left_maxDistance; i < endPos - startPos - right_maxDistance; i++)
                for (int j = 0; j < 5; j++) new_counts_gap(i)[j] = 0;
            GapString gapString = make_gap_string(new_bestString, gapLength);
            count_of_read = -1;
            for (size_t k = 0; k < prec->size(); k++) {
                const PartialRec &r = (*prec)[k];
                const string &rs = r.seq;
                int readLength1 = (int)rs.size();
                int flag1 = r.match, pos1 = r.pos, ref_pos = r.ref_pos, read_start, read_end;
                maxProb = -DBL_MAX; maxPos = 0;
                if (flag1 == 1 || flag1 == 4) { read_start = clip_thresh; read_end = 0; }
                else { read_start = 0; read_end = clip_thresh; }
                count_of_read++;
                if (count_of_read > (partial_limit - 1)) break;
                if (pos1 < gapStart) {
                    insertSize = (int)(gapStart - ref_pos + readLength1);
                    for (long i = gapStart - readLength1 + 1; i < gapStart; i++) {
                        tempInsertSize = (int)(insertSize + i - gapStart);
                        if ((tempInsertSize < M.insertThresholdMin || tempInsertSize > M.insertThresholdMax) && ref_pos != -1) continue;
                        tempProb = mle_product(rs, read_start, readLength1 - read_end, i, gapString, 0);
                        if (tempProb > maxProb) { maxProb = tempProb; maxPos = (int)(i - startPos); }
                    }
                } else {
                    if (ref_pos != -1) ref_pos += gapoffset;
                    insertSize = (int)(ref_pos - (gapStart + gapLength) + readLength1);
                    for (long i = gapStart + gapLength - readLength1 + 1; i < gapStart + gapLength; i++) {
                        tempInsertSize = (int)(insertSize + gapStart + gapLength - i);
                        if ((tempInsertSize < M.insertThresholdMin || tempInsertSize > M.insertThresholdMax) && ref_pos != -1) continue;
                        tempProb = mle_product(rs, read_start, readLength1 - read_end, i, gapString, 0);
                        if (tempProb > maxProb) { maxProb = tempProb; maxPos = (int)(i - startPos); }
                    }
                }
                double temp_log_val = -LM_LOG10(maxProb);
                if (count_of_read < partial_read_count) {
                    if (temp_log_val < M.gapProbCutOff) {
                        valid_count++;
                        pflag[count_of_read * 2 + 1] = maxPos - left_maxDistance;
                        if (gapLength == originalGap) {
                            partial_read_pos_arr_org[count_of_read * 3] = 1;
                            partial_read_pos_arr_org[count_of_read * 3 + 1] = maxPos - left_maxDistance;
                            partial_read_pos_arr_org[count_of_read * 3 + 2] = readLength1;
                        }
                    } else { invalid_count++; pflag[count_of_read * 2] = 0; }
                }
            }
            int ret_val[2] = {0, 0};
            detect_overlap_gapestimate(pflag.data(), 2, gapLength, ret_val, 8);
            if (ret_val[0] == 300) maxLikelihood += ret_val[0];
            else if (ret_val[0] >= 1 && ret_val[0] < MAX_READLENGTH) maxLikelihood += 30 * ret_val[0];
            else if (ret_val[1] == -1) maxLikelihood += -100;
            if (g_trace && g_trace_det)
                fprintf(g_trace, "DET\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\n", g, gapLength, ret_val[0], ret_val[1], partial_saved_read_temp[0],
                        partial_saved_read_temp[1], g_det_nmax, g_det_false, partial_read_count);
        }

        count_of_read = num_reads_in_gap;
        if (A.unmapped == 1) {
            for (int read_itr = 0; read_itr < count_of_read; read_itr++) {
                maxProb = -DBL_MAX; tempProb = 0; maxPos = 0;
                int pos1 = pos_reads[read_itr];
                const string &rs = reads_gap[read_itr];
                int readLength2 = (int)rs.size();
                if (pos1 < gapStart) {
                    insertSize = (int)(gapStart - pos1 + readLength2);
                    for (long i = gapStart - readLength2 + 1; i < gapStart + gapLength; i++) {
                        tempInsertSize = (int)(insertSize + i - gapStart);
                        if (tempInsertSize < M.insertThresholdMin || tempInsertSize > M.insertThresholdMax) continue;
                        tempProb = estep_product(M.insertLengthDistSmoothed[tempInsertSize], rs, 0, readLength2, i, isReverse[read_itr]);
                        tempProb = LM_LOG10(tempProb);
                        if (tempProb > maxProb) { maxProb = tempProb; maxPos = (int)(i - startPos); }
                        antilog_value = LM_EXP(0.5 * tempProb);
                        for (int j = 0; j < readLength2; j++)
                            if (i - startPos + j >= left_maxDistance && i - startPos + j < left_maxDistance + gapLength)
                                { countsGap(i - startPos + j)[cc(rs[j])] += antilog_value; g_flops += 1.0; }
                    }
                } else {
                    pos1 += gapoffset;
                    insertSize = (int)(pos1 - (gapStart + gapLength) + readLength2);
                    for (long i = gapStart - readLength2 + 1; i < gapStart + gapLength; i++) {
                        tempInsertSize = (int)(insertSize + gapStart + gapLength - i);
                        if (tempInsertSize < M.insertThresholdMin || tempInsertSize > M.insertThresholdMax) continue;
                        tempProb = estep_product(M.insertLengthDistSmoothed[tempInsertSize], rs, 0, readLength2, i, isReverse[read_itr]);
                        tempProb = LM_LOG10(tempProb);
                        if (tempProb > maxProb) { maxProb = tempProb; maxPos = (int)(i - startPos); }
                        antilog_value = LM_EXP(0.5 * tempProb);
                        for (int j = 0; j < readLength2; j++)
                            if (i - startPos + j >= left_maxDistance && i - startPos + j < left_maxDistance + gapLength)
                                { countsGap(i - startPos + j)[cc(rs[j])] += antilog_value; g_flops += 1.0; }
                    }
                }
                if (maxProb != -DBL_MAX) maxlikelihood_value[read_itr] = maxProb;
                else { maxlikelihood_value[read_itr] = 0; invalid_count++; }
            }
            if (g_trace && g_trace_level >= 3) {
                FILE *tf = trace_plane_file();
                fprintf(tf, "E\t%d\t%d\t%d", g, gapLength, ge);
                for (long i = left_maxDistance; i < left_maxDistance + gapLength; i++)
                    for (int j = 0; j < 5; j++) fprintf(tf, "\t%a", countsGap(i)[j]);
                fprintf(tf, "\nR\t%d\t%d\t%d", g, gapLength, ge);
                for (int r = 0; r < count_of_read; r++) fprintf(tf, "\t%a", maxlikelihood_value[r]);
                fprintf(tf, "\n");
            }
            computeSequence(0, 0);
            string new_bestString = concensus;
            for (long i = left_maxDistance; i < endPos - startPos - right_maxDistance; i++)
                for (int j = 0; j < 5; j++) new_counts_gap(i)[j] = 0;
            GapString gapString = make_gap_string(new_bestString, gapLength);
            for (int read_itr = 0; read_itr < count_of_read; read_itr++) {
                maxPos = 0; maxProb = -DBL_MAX;
                int pos1 = pos_reads[read_itr];
                const string &rs = reads_gap[read_itr];
                int readLength2 = (int)rs.size();
                if (pos1 < gapStart) {
                    insertSize = (int)(gapStart - pos1 + readLength2);
                    for (long i = gapStart - readLength2 + 1; i < gapStart + gapLength; i++) {
                        tempInsertSize = (int)(insertSize + i - gapStart);
                        if (tempInsertSize < M.insertThresholdMin || tempInsertSize > M.insertThresholdMax) continue;
                        tempProb = mle_product(rs, 0, readLength2, i, gapString, isReverse[read_itr]);
                        if (tempProb > maxProb) { maxProb = tempProb; maxPos = (int)(i - startPos); }
                    }
                } else {
                    pos1 += gapoffset;
                    insertSize = (int)(pos1 - (gapStart + gapLength) + readLength2);
                    for (long i = gapStart - readLength2 + 1; i < gapStart + gapLength; i++) {
                        tempInsertSize = (int)(insertSize + gapStart + gapLength - i);
                        if (tempInsertSize < M.insertThresholdMin || tempInsertSize > M.insertThresholdMax) continue;
                        tempProb = mle_product(rs, 0, readLength2, i, gapString, isReverse[read_itr]);
                        if (tempProb > maxProb) { maxProb = tempProb; maxPos = (int)(i - startPos); }
                    }
                }
                double temp_log_val = -LM_LOG10(maxProb);
                if (temp_log_val < M.gapProbCutOff) {
                    maxlikelihood_value[read_itr] = -temp_log_val;
                    maxLikelihood += maxlikelihood_value[read_itr];
                    valid_count++;
                } else maxLikelihood += -50;
                if (temp_log_val < M.gapProbCutOff) {
                    for (int j = 0; j < readLength2; j++)
                        if (maxPos + j >= left_maxDistance && maxPos + j < left_maxDistance + gapLength)
                            new_counts_gap(maxPos + j)[cc(rs[j])] += 1;
                    mark_accepted_reads[read_itr] = 1;
                    final_readpos[read_itr * 3] = maxPos - left_maxDistance;
                    final_readpos[read_itr * 3 + 1] = readLength2;
                    final_readpos[read_itr * 3 + 2] = read_itr;
                    if (gapLength == originalGap) {
                        unmapped_read_pos_arr_org[read_itr * 3] = maxPos - left_maxDistance;
                        unmapped_read_pos_arr_org[read_itr * 3 + 1] = readLength2;
                        unmapped_read_pos_arr_org[read_itr * 3 + 2] = read_itr;
                        fill_original = 1;
                    }
                    if (originalGap <= 30) {
                        int p0 = final_readpos[read_itr * 3], p1 = final_readpos[read_itr * 3 + 1];
                        int val = p0 + p1 - gapLength;
                        if (p0 < 0 && val > 0) { if (-p0 > 3 && val > 3) ucoverf = 1; }
                        if (p0 < 0 && p0 + p1 > 0) { if (-p0 > 3) umaxleftf = 1; }
                        if (p0 > 0 && p0 < gapLength && val > 0) { if (val > 3) umaxrightf = 1; }
                    }
                }
            }
            computeSequence(1, 1);
            current_str = concensus;
            if (current_str == previous_str) comp_count++;
            else { previous_str = current_str; comp_count = 0; }

            if (finalize_flag) {
                // coverage regions (:3935-3977)
                vector<int> region(50000, 0);
                int region_start = 0, region_count = 0;
                int region_left_right[2] = {MAX_GAP, -MAX_GAP};
                for (int i = 0; i < gapLength; i++) {
                    if (gap_coverage[i] < covergae_threshold2 && region_start == 0) { region[region_count] = i; region_start = 1; }
                    else if (gap_coverage[i] >= covergae_threshold2 && region_start == 1) {
                        if (i - 1 - region[region_count] >= 10) { region_start = 0; region[region_count + 1] = i - 1; region_count += 2; }
                    }
                    if (i == gapLength - 1 && region_start == 1) {
                        if (i - region[region_count] >= 10) { region_start = 0; region[region_count + 1] = i; region_count += 2; }
                    }
                }
                if (region_count) {
                    region_left_right[0] = region[0];
                    region_left_right[1] = region[region_count - 1];
                    region_perct = (region_left_right[1] - region_left_right[0] * 1.0) / gapLength;
                } else region_perct = 0;
                for (int i = 0; i < count_of_read; i++) {
                    if (mark_accepted_reads[i] == 1) {
                        if (final_readpos[i * 3] >= region_left_right[0] &&
                            final_readpos[i * 3] + final_readpos[i * 3 + 1] - 1 < region_left_right[1]) {
                            maxLikelihood += -50;
                            mark_accepted_reads[i] = 0;
                            if (gapLength == originalGap) { unmapped_read_pos_arr_org[i * 3] = -200; unmapped_read_pos_arr_org[i * 3 + 1] = 0; }
                            valid_count--;
                            final_readpos[i * 3] = -200; final_readpos[i * 3 + 1] = 0;
                        }
                    }
                }
                maxLikelihood += findOverlapUnmapped(final_readpos);
                int condition = A.unmapped && comp_count >= 1 && region_perct != 0 && ge != num_itr - 1;
                if (condition && updateflag) seed_reweight(count_of_read);
            }
        }
        return maxLikelihood;
    }

    // seed re-weighting (Figbird.cpp:4032-4376)
    void seed_reweight(int count_of_read) {
        vector<int> index_pair(1000, -1);
        int start_n = 0, pair_count = 0, start_index1, end_index1;
        int N_count = 0, num_match_count0 = 0, num_match_count1 = 1;
        int match_threshold = (int)(unmapped_read_len * 0.25);
        int max_segment_length = (int)(unmapped_read_len * 0.67);
        int min_gap_len = unmapped_read_len / 2 + 1;
        vector<double> count_pos((size_t)gapLength * 4, 0.0);
        int clen = (int)concensus.size();
        for (int i = 0; i < clen; i++) {
            if (concensus[i] == 'N' && start_n == 0) {
                start_n = 1;
                if (i > 0) index_pair[pair_count++] = i - 1; else index_pair[pair_count++] = i;
                N_count++;
            } else if (concensus[i] != 'N' && start_n == 1) {
                start_n = 0;
                index_pair[pair_count++] = i;
                if (N_count < min_gap_len) pair_count -= 2;
                N_count = 0;
            } else if (concensus[i] == 'N' && start_n == 1) N_count++;
            if (i == clen - 1 && start_n == 1) {
                index_pair[pair_count++] = i;
                if (N_count < min_gap_len) pair_count -= 2;
            }
        }
        if (pair_count > 2) index_pair[1] = index_pair[pair_count - 1];
        int flag1 = 1, flag2 = 1;
        if (pair_count < 2) { flag1 = 0; flag2 = 0; }
        if (!(flag1 == 1 || flag2 == 1)) return;
        end_index1 = index_pair[0];
        start_index1 = index_pair[1];
        int index_s = (end_index1 >= max_segment_length) ? end_index1 - max_segment_length + 1 : 0;
        string text_left, text_right;
        for (int j = index_s; j < clen && concensus[j] != 'N'; j++) text_left.push_back(concensus[j]);
        int stop_index = (start_index1 + max_segment_length <= clen) ? start_index1 + max_segment_length - 1 : clen - 1;
        for (int j = start_index1; j <= stop_index; j++) text_right.push_back(concensus[j]);
        const string str_arr[2] = {text_left, text_right};
        int temp_flag1 = flag1, temp_flag2 = flag2;
        for (int read_itr = 0; read_itr < count_of_read; read_itr++) {
            if (mark_accepted_reads[read_itr] == 0 && maxlikelihood_value[read_itr] != 0) {
                const string &rd = reads_gap[read_itr];
                int R2 = (int)rd.size();
                int mapped_pos = pos_reads[read_itr];
                flag1 = temp_flag1; flag2 = temp_flag2;
                for (int gg = 0; gg < 2; gg++) {
                    int placed_pos = (int)(gapStart + index_pair[gg]);
                    int insertsize;
                    if (mapped_pos < gapStart) insertsize = placed_pos + R2 - mapped_pos;
                    else insertsize = mapped_pos - placed_pos + R2;
                    if (insertsize < (M.insertThresholdMin) + 100 || insertsize > (M.insertThresholdMax - 100)) {
                        if (gg == 0) flag1 = 0; else flag2 = 0;
                    }
                }
                if (flag1 == 1) {
                    const string &sa = str_arr[0];
                    for (int j = 0; j < (int)sa.size(); j++) {
                        int match = 0, match_flag = 1;
                        for (int k = 0; k < (int)sa.size() - j; k++) {
                            char rc = k < R2 ? rd[k] : '\0';
                            if (sa[j + k] != rc) { match_flag = 0; break; } else match++;
                        }
                        if (match_flag == 1 && match > match_threshold) {
                            num_match_count0++;
                            for (int r = 0; r < R2; r++) {
                                int ind_read = cc(rd[r]);
                                int ind_ref = index_pair[0] - match + 1 + r;
                                if (ind_ref == gapLength) break;
                                if (ind_ref > index_pair[0]) {
                                    if (ind_read < 4) count_pos[ind_ref * 4 + ind_read] += match;
                                    else for (int q = 0; q < 4; q++) count_pos[ind_ref * 4 + q] += match;
                                }
                            }
                            break;
                        }
                    }
                }
                if (flag2 == 1) {
                    string temp_read_str(rd.rbegin(), rd.rend());
                    string temp_text_right(str_arr[1].rbegin(), str_arr[1].rend());
                    int tl = (int)temp_text_right.size();
                    for (int j = 0; j < tl; j++) {
                        int match = 0, match_flag = 1;
                        for (int k = 0; k < tl - j; k++) {
                            char rc = k < R2 ? temp_read_str[k] : '\0';
                            if (temp_text_right[j + k] != rc) { match_flag = 0; break; } else match++;
                        }
                        if (match_flag == 1 && match > match_threshold) {
                            num_match_count1++;
                            for (int r = 0; r < R2; r++) {
                                int ind_read = cc(rd[R2 - r - 1]);
                                int ind_ref = index_pair[1] + match - 1 - r;
                                if (ind_ref < 0) break;
                                if (ind_ref < index_pair[1]) {
                                    if (ind_ref >= gapLength) continue;   // out of count_pos in the reference (UB)
                                    if (ind_read < 4) count_pos[ind_ref * 4 + ind_read] += match;
                                    else for (int q = 0; q < 4; q++) count_pos[ind_ref * 4 + q] += match;
                                }
                            }
                            break;
                        }
                    }
                }
            }
        }
        // flag1/flag2 here hold the values left by the LAST examined read (:4310,4321)
        if (flag1 == 1 && num_match_count0 == 0 && index_pair[0] < (int)partial_left.size()) {
            for (int f = index_pair[0] + 1; f < (int)partial_left.size(); f++)
                if (f < gapLength) count_pos[f * 4 + cc(partial_left[f])] += 1;
        }
        if (flag2 == 1 && num_match_count1 == 0 && index_pair[1] > gapLength - (int)partial_right.size()) {
            for (int f = gapLength - (int)partial_right.size(), c = 0; f < index_pair[1]; f++)
                if (f >= 0 && f < gapLength) count_pos[f * 4 + cc(partial_right[c++])] += 1; else c++;
        }
        for (int j = 0; j < gapLength; j++) {
            int total_count_p = 0;
            for (int k = 0; k < 4; k++) total_count_p += count_pos[j * 4 + k];
            if (total_count_p > 0)
                for (int k = 0; k < 4; k++) countsGap(left_maxDistance + j)[k] = (count_pos[j * 4 + k] / total_count_p);
        }
    }

    // ------------------------------------------------------------------ computeSequence :4417-4508
    void computeSequence(int check, int choice_array) {
        long index = endPos - startPos - (left_maxDistance + right_maxDistance);
        if (index < 0) index = 0;
        concensus.assign((size_t)index, 'N');
        for (long i = left_maxDistance; i < endPos - startPos - right_maxDistance; i++) {
            double mx = 0; int maxIndex = -1, flag = 0;
            for (int j = 0; j <= 4; j++) {
                double v = choice_array == 0 ? countsGap(i)[j] : new_counts_gap(i)[j];
                if (v > mx) { mx = v; maxIndex = j; flag = 1; }
            }
            int coverage_flag = 1;
            if (check == 1) {
                gap_coverage[i - left_maxDistance] = (int)mx;
                if (gap_coverage[i - left_maxDistance] <= covergae_threshold1) coverage_flag = 0;
            }
            char c;
            if (((flag == 1) || (!check)) && coverage_flag)
                c = maxIndex == 0 ? 'A' : maxIndex == 1 ? 'C' : maxIndex == 2 ? 'G' : maxIndex == 3 ? 'T' : 'N';
            else c = 'N';
            concensus[i - left_maxDistance] = c;
        }
    }

    int checkAllZero(double *arr, int flag) {               // :4524-4533
        int non_zero = 0;
        for (int k = 0; k < 4; k++) if (arr[k] > flag) non_zero++;
        return non_zero == 0 ? 0 : 1;
    }

    int check_update(double *arr, int j) {                  // :4535-4581
        double max_val = -DBL_MAX, second_max = -DBL_MAX;
        int maxp = -MAX_GAP, sec_p = -MAX_GAP;
        for (int k = 0; k < 4; k++) {
            if (arr[k] > max_val) { second_max = max_val; sec_p = maxp; max_val = arr[k]; maxp = k; }
            else if (arr[k] >= second_max) { second_max = arr[k]; sec_p = k; }
        }
        int diff = (int)(max_val - second_max);
        if (diff >= partial_threshold) {
            if (max_val > 3 && second_max > 3) {
                if (qual_gap(j)[maxp] <= qual_gap(j)[sec_p]) return maxp; else return sec_p;
            }
            return 50;
        } else {
            if (max_val >= 1 && second_max >= 1) {
                if (qual_gap(j)[maxp] <= qual_gap(j)[sec_p]) return maxp; else return sec_p;
            }
            return -1;
        }
    }

    void clear_countsGap(int a) {                           // :4583-4592
        for (int j = 0; j < a; j++) for (int k = 0; k < 4; k++) countsGap(j + left_maxDistance)[k] = 0;
    }

    int findRegion(vector<int> &region) {                   // :4594-4621
        int Nstart = 0, region_count = 0, len = gapLength;
        region.assign(5000 + 2 * (size_t)len + 4, 0);
        for (int i = 0; i < len; i++) {
            char c = (size_t)i < concensus.size() ? concensus[i] : '\0';
            if (c == 'N' && Nstart == 0) { region[2 * region_count] = i; Nstart = 1; }
            else if (c != 'N' && Nstart == 1) { Nstart = 0; region[2 * region_count + 1] = i - 1; region_count++; }
            if (i == len - 1 && Nstart == 1) { region[2 * region_count + 1] = i; region_count++; }
        }
        return region_count;
    }

    int findDiscontinous(vector<int> &pos, vector<int> &rv) {   // :4623-4666
        vector<Trip> vec(num_reads_in_gap);
        for (int i = 0; i < num_reads_in_gap; i++) for (int j = 0; j < 3; j++) vec[i].v[j] = pos[i * 3 + j];
        std::sort(vec.begin(), vec.end(), sortcol);
        int diff, discount = 0;
        for (int i = 0; i < num_reads_in_gap - 1; i++) {
            if (vec[i].v[0] != -200) {
                diff = (vec[i].v[0] + vec[i].v[1] - vec[i + 1].v[0]);
                if (diff >= 0 && diff <= match_count_discont / 2) rv.push_back(vec[i].v[0] + vec[i].v[1]);
            }
        }
        discount = (int)rv.size();
        return discount;
    }

    void set_cons(long idx, char c) {                       // concensus[idx]=c on a maxGap+1 buffer
        if (idx < 0) return;
        if ((size_t)idx < concensus.size()) concensus[idx] = c;
        // idx >= length: the reference writes at/after the terminator; invisible to every later
        // reader (all of them are bounded by gapLength).
    }

    int recheck_sequence(vector<int> &pos) {                // :4668-4743
        vector<int> region;
        int region_count = findRegion(region);
        int len = gapLength;
        vector<int> nec_ret;
        int flag = findDiscontinous(pos, nec_ret);
        if (flag > 0) {
            for (int k = 0; k < flag; k++) set_cons(nec_ret[k], 'N');
            region_count = findRegion(region);
        }
        double reduction_factor = originalGap < 400 ? 1 : originalGap < 1200 ? 1.5 : 2;
        int readchar = 30;
        if (region_count <= 1) {
            if (region_count == 1) {
                if (region_perct_max_gap_estm < .75 || flag > 0) {
                    int i, j;
                    for (i = region[0] - 1; i >= region[0] - reduction_factor * readchar && i >= 0; i--) set_cons(i, 'N');
                    for (j = region[1] + 1; j <= region[1] + reduction_factor * readchar && j < len; j++) set_cons(j, 'N');
                    if (i < 0 && j == len) return 1;
                }
            }
        } else {
            int start = region[0], end = region[2 * region_count - 1];
            for (int j = start; j < end; j++) set_cons(j, 'N');
            int i, j;
            for (i = start - 1; i > start - 1 - reduction_factor * readchar && i >= 0; i--) set_cons(i, 'N');
            for (j = end + 1; j < end + 1 + reduction_factor * readchar && j < len; j++) set_cons(j, 'N');
            if (i < 0 && j == len) {
                gapLength = originalGap;
                initialize_start_end();
                return 1;
            }
        }
        return 0;
    }

    void recompute1(vector<int> &position) {                // :4875-4906
        int read_itr = 0;
        for (size_t k = 0; k < prec->size(); k++) {
            const string &rs = (*prec)[k].seq;
            if ((size_t)read_itr * 3 < position.size() && position[read_itr * 3] == 1) {
                int pos = position[read_itr * 3 + 1];
                for (int j = 0; j < (int)rs.size(); j++)
                    if (pos + j >= 0 && pos + j < gapLength) countsGap(pos + j + left_maxDistance)[cc(rs[j])] += 1;
            }
            read_itr++;
            if (read_itr > partial_limit) break;
        }
    }

    void recompute2(vector<int> &position) {                // :4908-4927
        for (int read_itr = 0; read_itr < num_reads_in_gap; read_itr++) {
            if (position[read_itr * 3 + 1] > 0) {
                int pos = position[read_itr * 3];
                const string &rs = reads_gap[read_itr];
                for (int j = 0; j < (int)rs.size(); j++)
                    if (pos + j >= 0 && pos + j < gapLength) countsGap(pos + j + left_maxDistance)[cc(rs[j])] += 1;
            }
        }
    }

    // ------------------------------------------------------------------ finalize :4929-5659
    void finalize(int gl, int gapno) {
        int gapoffset = gl - originalGap;
        vector<int> partial_read_flag((size_t)partial_read_count * 3);
        for (int i = 0; i < partial_read_count; i++) {
            partial_read_flag[i * 3] = 0; partial_read_flag[i * 3 + 1] = -200; partial_read_flag[i * 3 + 2] = partial_read_len;
        }
        double maxProb = 0, tempProb;
        vector<int> unmapped_read_pos_arr((size_t)num_reads_in_gap * 3);
        for (int i = 0; i < num_reads_in_gap; i++) {
            unmapped_read_pos_arr[i * 3] = -200; unmapped_read_pos_arr[i * 3 + 1] = 0; unmapped_read_pos_arr[i * 3 + 2] = -1;
        }
        int insertSize, mleInsertSize = 0, tempInsertSize;
        int left_right_check[2] = {0, 0};
        int leftcount = 0, rightcount = 0, left_start_zero = 0, right_fin_glen = 0;
        int maxPos, totalCount = 0, discardedCount = 0;
        int unmapped_max_left = 0, unmapped_max_right = 0;
        // gapString is built with the CURRENT left/right_maxDistance/startPos, before gapLength is reset (:4978-4996)
        GapString gapString = make_gap_string(bestString, gl);
        long end_lim = left_maxDistance + alloc_arg;
        for (long i = left_maxDistance; i < end_lim && i < end_pos_max; i++) {
            if (i >= maxSize) break;
            for (int j = 0; j < 5; j++) countsGap(i)[j] = 0;
        }
        gapLength = gl;
        initialize_start_end();

        if (A.unmapped) {
            draw_read(gapLength, "S", 0, 0, gapno, ' ');
            for (int read_itr = 0; read_itr < num_reads_in_gap; read_itr++) {
                maxProb = 0; maxPos = 0;
                totalCount++;
                int pos1 = pos_reads[read_itr];
                const string &rs = reads_gap[read_itr];
                int readLength2 = (int)rs.size();
                if (pos1 < gapStart) {
                    insertSize = (int)(gapStart - pos1 + readLength2);
                    for (long i = gapStart - readLength2 + 1; i < gapStart + gapLength; i++) {
                        tempInsertSize = (int)(insertSize + i - gapStart);
                        if (tempInsertSize < M.insertThresholdMin || tempInsertSize > M.insertThresholdMax) continue;
                        tempProb = mle_product(rs, 0, readLength2, i, gapString, isReverse[read_itr]);
                        if (tempProb > maxProb) { maxProb = tempProb; mleInsertSize = (int)(insertSize + i - gapStart); maxPos = (int)(i - startPos); }
                    }
                } else {
                    pos1 += gapoffset;
                    insertSize = (int)(pos1 - (gapStart + gapLength) + readLength2);
                    for (long i = gapStart - readLength2 + 1; i < gapStart + gapLength; i++) {
                        tempInsertSize = (int)(insertSize + gapStart + gapLength - i);
                        if (tempInsertSize < M.insertThresholdMin || tempInsertSize > M.insertThresholdMax) continue;
                        tempProb = mle_product(rs, 0, readLength2, i, gapString, isReverse[read_itr]);
                        if (tempProb > maxProb) { maxProb = tempProb; mleInsertSize = (int)(insertSize + gapStart + gapLength - i); maxPos = (int)(i - startPos); }
                    }
                }
                if (-LM_LOG10(maxProb) < M.gapProbCutOff && saved_reads[read_itr] == 1) {
                    char ifelse = (pos1 < gapStart) ? 'I' : 'E';
                    draw_read(maxPos - left_maxDistance, rs.c_str(), read_itr, mleInsertSize, gapno, ifelse);
                    int p = maxPos - left_maxDistance;
                    unmapped_read_pos_arr[read_itr * 3] = p;
                    unmapped_read_pos_arr[read_itr * 3 + 1] = readLength2;
                    unmapped_read_pos_arr[read_itr * 3 + 2] = read_itr;
                    if (p == 0) left_start_zero = 1;
                    if (p + readLength2 == gapLength) right_fin_glen = 1;
                    if (p < 0 && p + readLength2 > 0) { left_right_check[0] = 1; if (-p > unmapped_max_left) unmapped_max_left = -p; }
                    int val = p + readLength2 - gapLength;
                    if (p < gapLength && val > 0) { left_right_check[1] = 1; if (val > unmapped_max_right) unmapped_max_right = val; }
                    for (int j = 0; j < readLength2; j++)
                        if (maxPos + j >= left_maxDistance && maxPos + j < left_maxDistance + gl)
                            countsGap(maxPos + j)[cc(rs[j])] += 1;
                } else discardedCount++;
            }
        }

        if (A.partial_flag) {
            int read_itr = -1;
            draw_read(gapLength, "S", 0, 0, gapno, ' ');
            for (size_t k = 0; k < prec->size(); k++) {
                const PartialRec &r = (*prec)[k];
                const string &rs = r.seq;
                int newInsertSize = -1;
                int readLength1 = (int)rs.size();
                int flag1 = r.match, pos1 = r.pos, ref_pos = r.ref_pos, read_start, read_end;
                maxProb = 0; maxPos = 0;
                totalCount++;
                if (flag1 == 1 || flag1 == 4) { read_start = clip_thresh; read_end = 0; }
                else { read_start = 0; read_end = clip_thresh; }
                read_itr++;
                if (read_itr > (partial_limit - 1)) break;
                if (pos1 < gapStart) {
                    insertSize = (int)(gapStart - ref_pos + readLength1);
                    for (long i = gapStart - readLength1 + 1; i < gapStart; i++) {
                        tempInsertSize = (int)(insertSize + i - gapStart);
                        if ((tempInsertSize < M.insertThresholdMin || tempInsertSize > M.insertThresholdMax) && ref_pos != -1) continue;
                        tempProb = mle_product(rs, read_start, readLength1 - read_end, i, gapString, 0);
                        if (tempProb > maxProb) { maxProb = tempProb; maxPos = (int)(i - startPos); }
                    }
                } else {
                    ref_pos += gapoffset;                   // no `!= -1` guard here (:5295)
                    insertSize = (int)(ref_pos - (gapStart + gapLength) + readLength1);
                    for (long i = gapStart + gapLength - readLength1 + 1; i < gapStart + gapLength; i++) {
                        tempInsertSize = (int)(insertSize + gapStart + gapLength - i);
                        if ((tempInsertSize < M.insertThresholdMin || tempInsertSize > M.insertThresholdMax) && ref_pos != -1) continue;
                        tempProb = mle_product(rs, read_start, readLength1 - read_end, i, gapString, 0);
                        if (tempProb > maxProb) { maxProb = tempProb; maxPos = (int)(i - startPos); }
                    }
                }
                if (-LM_LOG10(maxProb) < M.gapProbCutOff || partial_saved_read_final[0] == read_itr || partial_saved_read_final[1] == read_itr) {
                    int p = maxPos - left_maxDistance;
                    if (p < 0) leftcount++; else rightcount++;
                    if (p < 0 && p + readLength1 >= gapLength)
                        if (-p >= 3 && (p + readLength1 - gapLength) >= 3) leftcount = rightcount = 10;
                    if (read_itr < partial_read_count) {
                        partial_read_flag[read_itr * 3] = 1; partial_read_flag[read_itr * 3 + 1] = p; partial_read_flag[read_itr * 3 + 2] = readLength1;
                    }
                    int placed_pos = (int)(p + gapStart);
                    if (p < 0) { if (ref_pos != -1) newInsertSize = placed_pos - ref_pos + readLength1; }
                    else { if (ref_pos != -1) newInsertSize = ref_pos + readLength1 - placed_pos; }
                    draw_read(p, rs.c_str(), read_itr, newInsertSize, gapno, 'P');
                    for (int j = 0; j < readLength1; j++)
                        if (maxPos + j >= left_maxDistance && maxPos + j < left_maxDistance + gl) {
                            countsGap(maxPos + j)[cc(rs[j])] += 1;
                            double q = 0;
                            if ((size_t)read_itr < partial_read_quality.size() && (size_t)j < partial_read_quality[read_itr].size())
                                q = partial_read_quality[read_itr][j];
                            qual_gap(maxPos + j - left_maxDistance)[cc(rs[j])] += q;
                        }
                } else discardedCount++;
            }
        }

        int used_read = totalCount - discardedCount, recompute_flag = 0;
        int Nflag[2] = {-1, -1}, lflag[2] = {-1, -1};
        int unmapped_sidethresh;
        if (A.unmapped == 1) {
            unmapped_sidethresh = 4;
            if ((unmapped_max_left < 2 * unmapped_sidethresh && unmapped_max_left > 0) ||
                (unmapped_max_right < 2 * unmapped_sidethresh && unmapped_max_right > 0)) {
                if (region_perct_max_gap_estm > .75) used_read = 0;
            }
            if ((unmapped_max_left < unmapped_sidethresh && unmapped_max_left > 0) ||
                (unmapped_max_right < unmapped_sidethresh && unmapped_max_right > 0)) {
                vector<int> region;
                computeSequence(1, 0);
                int rc = findRegion(region);
                if (rc >= 1) {
                    if (unmapped_max_left < unmapped_sidethresh && unmapped_max_left > 0) lflag[0] = 1;
                    if (unmapped_max_right < unmapped_sidethresh && unmapped_max_right > 0) lflag[1] = 1;
                } else if (rc == 0) { used_read = 0; unmapped_max_left = unmapped_max_right = -1; }
            }
            if (left_right_check[0] == 0 && left_right_check[1] == 0 && used_read != 0) {
                used_read = 0; unmapped_max_left = unmapped_max_right = -1;
            }
            if ((left_right_check[0] == 0 && left_start_zero != 0) || (left_right_check[1] == 0 && right_fin_glen != 0)) {
                vector<int> region;
                computeSequence(1, 0);
                int rc = findRegion(region);
                if (rc >= 1) { if (left_right_check[0] == 0) Nflag[0] = 1; if (left_right_check[1] == 0) Nflag[1] = 1; }
            }
            if (used_read == 0 || (!(left_right_check[0] == 1 && left_right_check[1] == 1))) {
                gapLength = originalGap;
                initialize_start_end();
                int offset = gapLength > gl ? 0 : (gl - gapLength);
                clear_countsGap(gapLength + offset);
                if (!left_right_check[0] && left_right_check[1] && unmapped_max_right >= unmapped_sidethresh) {
                    recompute2(unmapped_read_pos_arr_org); recompute_flag = 1;
                } else if (left_right_check[0] && !left_right_check[1] && unmapped_max_left >= unmapped_sidethresh) {
                    recompute2(unmapped_read_pos_arr_org); recompute_flag = 1;
                }
            }
        }
        if (A.partial_flag == 1) {
            int ret_val[2] = {0, 0};
            int u_flag = 1;
            detect_overlap_gapestimate(partial_read_flag.data(), 3, gapLength, ret_val, 8);
            int gap_case;
            if ((originalGap - gl) > 0 && ret_val[0] > 0) gap_case = 1;
            else if ((originalGap - gl) > 0 && ret_val[0] == 0) gap_case = 2;
            else if ((originalGap - gl) < 0 && ret_val[0] > 0) gap_case = 3;
            else if ((originalGap - gl) < 0 && ret_val[0] == 0) gap_case = 4;
            else gap_case = 5;
            if (used_read < partial_threshold || gap_case == 2 || gap_case == 4) {
                gapLength = originalGap;
                initialize_start_end();
                int offset = gapLength > gl ? 0 : (gl - gapLength);
                clear_countsGap(gapLength + offset);
                if (used_read < partial_threshold || gap_case == 4) u_flag = 0;
                else {
                    recompute1(partial_read_pos_arr_org);
                    for (int i = 0; i < partial_read_count; i++)
                        for (int q = 0; q < 3; q++) partial_read_flag[i * 3 + q] = partial_read_pos_arr_org[i * 3 + q];
                    detect_overlap_gapestimate(partial_read_flag.data(), 3, gapLength, ret_val, 8);
                    if (ret_val[1] == -1) { clear_countsGap(gapLength + offset); u_flag = 0; }
                }
            }
            if (u_flag == 1 && ret_val[0] == 0 && ret_val[1] == 0) {
                for (int j = 0; j < gapLength; j++) {
                    if (checkAllZero(countsGap(j + left_maxDistance), 0) == 1) {
                        int update_flag = check_update(countsGap(j + left_maxDistance), j);
                        if (update_flag != -1) { if (update_flag != 50) countsGap(j + left_maxDistance)[update_flag] += 10; }
                        else for (int k = 0; k < 4; k++) countsGap(j + left_maxDistance)[k] = 0;
                    }
                }
            }
        }
        computeSequence(1, 0);
        if ((A.unmapped && (left_right_check[0] || left_right_check[1] || used_read != 0))) {
            if (Nflag[0] == 1) set_cons(0, 'N');
            if (Nflag[1] == 1) set_cons(gapLength - 1, 'N');
            if (lflag[0] == 1) set_cons(0, 'N');
            if (lflag[1] == 1) set_cons(gapLength - 1, 'N');
            int clear_val;
            if (recompute_flag == 0) clear_val = recheck_sequence(unmapped_read_pos_arr);
            else clear_val = recheck_sequence(unmapped_read_pos_arr_org);
            if (clear_val == 1) {
                gapLength = originalGap;
                initialize_start_end();
                int offset = gapLength > gl ? 0 : (gl - gapLength);
                clear_countsGap(gapLength + offset);
                computeSequence(1, 0);
            }
        }
    }

    // ------------------------------------------------------------------ parseUnmapped :5661-5767
    void parseUnmapped(int g) {
        int r_c = 0, total_read = 0;
        max_read_len = 0;
        size_t li = 0;
        const vector<string> &ln = *ulines;
        while (li < ln.size()) {
            const string &line1 = ln[li++];
            if (!line1.empty() && line1[0] == '@') continue;
            if (line1.size() < 60) { printf("unknown problem in sam, skipping read no - %d for gap - %d\n", r_c, g); continue; }
            if (li >= ln.size()) break;
            const string &line2 = ln[li++];
            if (r_c >= num_reads_in_gap) break;             // reference would overflow its arrays
            vector<char> b1(line1.begin(), line1.end()); b1.push_back('\0');
            vector<char> b2(line2.begin(), line2.end()); b2.push_back('\0');
            char *sv = nullptr;
            strtok_r(b1.data(), "\t", &sv);
            char *temp = strtok_r(NULL, "\t", &sv);
            int flag = temp ? atoi(temp) : 0;
            int strandNo1 = (flag & 16) >> 4;
            strtok_r(NULL, "\t", &sv);
            temp = strtok_r(NULL, "\t", &sv);
            pos_reads[r_c] = temp ? atoi(temp) : 0;
            sv = nullptr;
            strtok_r(b2.data(), "\t", &sv);
            strtok_r(NULL, "\t", &sv);
            for (int j = 0; j < 4; j++) strtok_r(NULL, "\t", &sv);
            char *readString2 = strtok_r(NULL, "\t", &sv);
            string rs = readString2 ? readString2 : "";
            if ((int)rs.size() > max_read_len) max_read_len = (int)rs.size();
            int rev_flag;
            if (strandNo1 == 0) {                           // reverse(), Figbird.cpp:1427-1449
                string t(rs.size(), 'N');
                int n = (int)rs.size();
                for (int i = 1; i <= n; i++) {
                    char ch = rs[i - 1], o;
                    if (ch == 'A' || ch == 'a') o = 'T'; else if (ch == 'C' || ch == 'c') o = 'G';
                    else if (ch == 'G' || ch == 'g') o = 'C'; else if (ch == 'T' || ch == 't') o = 'A'; else o = 'N';
                    t[n - i] = o;
                }
                rs = t; rev_flag = 1;
            } else rev_flag = 0;
            reads_gap[r_c] = rs;
            isReverse[r_c] = rev_flag;
            r_c++;
            total_read++;
            if (total_read == unmapped_limit) break;
        }
    }

    // ------------------------------------------------------------------ parsePartial :5769-5842 (+qualityFilter :1780-1797)
    void parsePartial() {
        int countp = 0;
        if (A.partial_flag) countp = partial_read_count;
        else { for (size_t k = 0; k < prec->size(); k++) { countp++; if (countp > partial_limit) break; } }
        p_count = countp;
        if (p_count > 0 && A.partial_flag) {
            partial_read_quality.assign(partial_read_count, vector<double>());
            countp = 0;
            for (size_t k = 0; k < prec->size(); k++) {
                if (countp >= partial_read_count) break;
                string q = (*prec)[k].qual;
                if ((int)q.size() > partial_read_len) q.resize(partial_read_len);   // token[partial_read_len]='\0'
                vector<double> &dst = partial_read_quality[countp];
                dst.assign(std::max((size_t)partial_read_len, q.size()), 0.0);
                for (size_t i = 0; i < q.size(); i++) {
                    int Q = q[i] - 33;
                    dst[i] = pow(10, -Q / 10.0);
                }
                countp++;
                if (countp > partial_limit) break;
            }
        }
    }

    // ------------------------------------------------------------------ run :5913-5965
    double run(int gaplen, int g, int finalize_flag, int c) {
        double likelihood = 0;
        left_maxDistance = A.D; right_maxDistance = A.D;
        initialize(gaplen, 1, 1);
        if (side_limit < 10) return 10000;
        step2match = 0;
        comp_count = 0;
        int p;
        for (p = 0; p < num_itr; p++) {
            valid_count = 0; invalid_count = 0;
            likelihood = placeReads(p, g, finalize_flag, gaplen - originalGap, 0);
            computeProbsGap(0);
            computeErrorProbsGap();
            if (A.unmapped) { if (comp_count >= 5) break; }
            else { if (p == 2) break; }
        }
        region_perct_max_gap_estm = region_perct;
        double retvall = 0;
        if (c == 0) retvall = valid_count;
        if (c == 1) retvall = likelihood;
        return retvall;
    }

    int checkGapReads(int org, int g) {                     // :6121-6153
        int readcountThresh = 3;
        if (org < 30) {
            int step = org < 15 ? 10 : 20;
            for (int i = 0; i < 80; i += step) {
                double val = run(i, g, 1, 1);
                if (val == 10000) return -2;
                if (valid_count > readcountThresh) return -1;
            }
        } else {
            for (int k = 0; k < 4; k++) {
                int gap = k == 0 ? org / 2 : org * k;
                double val = run(gap, g, 1, 1);
                if (val == 10000) return -2;
                if (valid_count >= readcountThresh) return -1;
            }
        }
        return 1;
    }

    void setParameters() {                                  // :6157-6165
        covergae_threshold1 = 0; match_count_discont = 4; covergae_threshold2 = 1;
        partial_threshold = 2; clip_thresh = 2;
    }

    void analyzeGap(int *g, int fillflag) {                 // :6168-6199
        findGapLeftRight();
        rep_flag = findRepeat();
        if (rep_flag == 1 && A.partial_flag) { g[0] = -1; g[1] = -1; }
        else if (one_side_repeat_flag == 1 && A.partial_flag && originalGap > 3 * mid_limitp) { g[0] = -1; g[1] = -1; }
        else if (fillflag == -1) { g[0] = -1; g[1] = -1; }
        else {
            if (partial_read_count == 0 && num_reads_in_gap == 0) { g[0] = -1; g[1] = -1; }
            else { if (A.script_itr == 1) { g[0] = 0; g[1] = 765466; } else { g[0] = 0; g[1] = 965757; } }
        }
    }

    static int check_change(const vector<int> &arr, int n) {    // :5886-5895
        if (n == 1) return 0;
        for (int i = 1; i < n; i++) if (arr[0] != arr[i]) return 1;
        return 0;
    }

    // ------------------------------------------------------------------ fillGap :6201-6570
    void fillGap(int g, int fillflag) {
        int finalize_flag = 1, gnum1, gnum2;
        int gapnum[2];
        if (A.unmapped) { if (large_gap_flag == 0) finalize_flag = 0; }
        if (A.unmapped) parseUnmapped(g);
        parsePartial();
        setParameters();
        analyzeGap(gapnum, fillflag);
        gnum1 = gapnum[0]; gnum2 = gapnum[1];
        bool inr = (g >= gnum1 && g <= gnum2);
        num_itr = inr ? 200 : 0;
        if (!inr) { gp_frac1 = 1; gp_frac2 = 1; }
        int gapMin = (int)(originalGap * gp_frac1);
        int gapMax = (int)(originalGap * gp_frac2);
        int gapEstimate = gapMin, maxGapEstimate = gapMin;
        double maxLikelihood = -DBL_MAX, secondMaxLikelihood = -DBL_MAX;
        double likelihood = 0, prevlikelihood = 0;
        bestString.clear(); secondBestString.clear(); current_str.clear(); previous_str.clear();
        string original_str;                                 // uninitialised VLA in the reference (:6255)
        int fill_or_not = 0;
        int same_count = 0, partial_same = 4, jump_same = 50, same_thresh;
        int stuckCount = 0;
        same_thresh = A.unmapped ? jump_same : partial_same;
        int range = gapMax - gapMin + 1;
        vector<int> used_read_arr(std::max(range, 1), 0);
        double diff1 = 0;
        int side_flag = 0, j = 0;
        vector<int> lrmd((size_t)std::max(range, 1) * 2, 0);
        int less_read_flag = 0;
        if (A.unmapped && originalGap <= mid_limitu && inr) less_read_flag = checkGapReads(originalGap, g);
        if (less_read_flag == 1) range = 0;
        if (less_read_flag == -2) { side_flag = 1; range = 0; }
        int prev_best = -1, curr_best = 0, prev_u = -1, curr_u = 0, sec_same = 0, sec_same2 = 0;

        for (; j < range; j++) {
            umaxleftf = umaxrightf = ucoverf = 0;
            fill_or_not = initialize(gapEstimate, 1, j);
            if (side_limit < 10) { side_flag = 1; break; }
            if (one_side_repeat_flag == 1) fill_or_not = 0;
            if (fill_or_not != 0 && inr) break;
            int i = 0;
            discont_or_not = 0;
            int preset_unfilled_len = 2 * unmapped_read_len;
            comp_count = 0;
            overlap_threshold = 5;
            step2match = 0;
            for (i = 0; i < num_itr; i++) {
                valid_count = 0; invalid_count = 0;
                likelihood = placeReads(i, g, finalize_flag, gapEstimate - originalGap, large_gap_flag);
                computeProbsGap(0);
                computeErrorProbsGap();
                if (g_trace && g_trace_level >= 2)
                    fprintf(g_trace, "IT\t%d\t%d\t%d\t%a\t%d\t%d\t%s\n", g, gapEstimate, i, likelihood, valid_count, comp_count, current_str.c_str());
                if (A.unmapped) {
                    if (comp_count >= 5) break;
                    if (large_gap_flag == 1 && region_perct * gapEstimate < preset_unfilled_len) break;
                } else { if (i == 2) break; }
            }
            if (A.unmapped && !finalize_flag && inr) {
                valid_count = 0;
                likelihood = placeReads(i, g, 1, gapEstimate - originalGap, 0);
            }
            computeSequence(0, 0);
            if (g_trace && g_trace_level >= 1) {
                trace_plane_flush();
                fprintf(g_trace, "CAND\t%d\t%d\t%d\t%a\t%d\t%s\n", g, gapEstimate, i, likelihood, valid_count, concensus.c_str());
            }
            if (likelihood > maxLikelihood) {
                secondMaxLikelihood = maxLikelihood;
                secondBestString = bestString;
                maxLikelihood = likelihood;
                maxGapEstimate = gapEstimate;
                bestString = concensus;
                for (int k = 0; k < num_reads_in_gap; k++) saved_reads[k] = mark_accepted_reads[k];
                region_perct_max_gap_estm = region_perct;
                for (int k = 0; k < 2; k++) partial_saved_read_final[k] = partial_saved_read_temp[k];
                curr_best = j;
                prev_u = valid_count;
            } else if (likelihood > secondMaxLikelihood) {
                secondMaxLikelihood = likelihood;
                secondBestString = concensus;
            }
            lrmd[j * 2] = left_maxDistance; lrmd[j * 2 + 1] = right_maxDistance;
            if (gapEstimate == originalGap) original_str = concensus;
            if (A.partial_flag || A.unmapped) {
                used_read_arr[j] = valid_count;
                diff1 = std::abs(prevlikelihood - likelihood);
                if (diff1 <= 0.9) same_count++; else same_count = 0;
                prevlikelihood = likelihood;
                if (same_count == same_thresh && gapLength >= originalGap) break;
                else if (same_count == same_thresh && gapLength < originalGap) {
                    run(originalGap, g, 1, 0);
                    computeSequence(0, 0);
                    original_str = concensus;
                    break;
                }
                if (A.unmapped) {
                    curr_u = valid_count;
                    if (curr_best == prev_best && std::abs(curr_u - prev_u) <= 2) sec_same++;
                    else { prev_best = curr_best; sec_same = 0; }
                    if (sec_same >= 2 * same_thresh) {
                        if (gapLength >= originalGap) break;
                        else { run(originalGap, g, 1, 0); computeSequence(0, 0); original_str = concensus; break; }
                    }
                    if (originalGap <= 30) {
                        if (!(umaxleftf == 1 || umaxrightf == 1 || ucoverf == 1)) sec_same2++; else sec_same2 = 0;
                        if (sec_same2 >= 1.5 * same_thresh) {
                            if (gapLength >= originalGap) break;
                            else { run(originalGap, g, 1, 0); computeSequence(0, 0); original_str = concensus; break; }
                        }
                    }
                    if (discont_or_not == 1 && valid_count < 5) stuckCount++; else stuckCount = 0;
                    if (stuckCount > 3 * same_thresh) {
                        if (gapLength >= originalGap) break;
                        else { run(originalGap, g, 1, 0); computeSequence(0, 0); original_str = concensus; break; }
                    }
                }
            }
            gapEstimate++;
        }

        if (fill_or_not != 0 && inr) {
            gapLength = 0;
            gaptofill[g] = fill_or_not;
        } else if (inr) {
            if (A.unmapped) {
                if (less_read_flag == 1) {
                    run(originalGap, g, 1, 0);
                    computeSequence(0, 0);
                    original_str = concensus;
                    finalize(originalGap, g);
                } else if (side_flag) {
                    run(originalGap, g, 1, 0);
                    computeSequence(0, 0);
                    bestString = concensus;
                    finalize(originalGap, g);
                } else if (check_change(used_read_arr, j) == 1) {
                    finalize(maxGapEstimate, g);
                } else {
                    bestString = original_str;
                    finalize(originalGap, g);
                }
            } else {
                if (maxGapEstimate == 0) {
                    if (used_read_arr[maxGapEstimate] != 0) finalize(maxGapEstimate, g);
                    else {
                        if (maxGapEstimate < originalGap) { run(originalGap, g, 1, 0); computeSequence(0, 0); original_str = concensus; }
                        finalize(originalGap, g);
                    }
                } else {
                    if (side_flag) {
                        int idx = maxGapEstimate - gapMin;
                        if (idx >= 0 && (size_t)idx * 2 + 1 < lrmd.size()) { left_maxDistance = lrmd[idx * 2]; right_maxDistance = lrmd[idx * 2 + 1]; }
                    }
                    finalize(maxGapEstimate, g);
                }
            }
        }
        if (g_trace && g_trace_level >= 1)
            fprintf(g_trace, "FINAL\t%d\t%d\t%d\t%s\n", g, gapLength, gaptofill[g], concensus.substr(0, std::min((size_t)gapLength, concensus.size())).c_str());
    }
};

// findFrac, Figbird.cpp:6879-6906
static int findFrac(int originalGap, float *info, int mid_limitp, int mid_limitu) {
    int ret_val;
    if (A.partial_flag) {
        if (originalGap <= mid_limitp / 2) { info[0] = .00001; info[1] = (float)factor_g / originalGap; ret_val = -1; }
        else if (originalGap <= mid_limitp) { info[0] = .00001; info[1] = 5.0; ret_val = 5; }
        else { info[0] = 1; info[1] = 1; ret_val = 3; }
    } else {
        if (originalGap <= mid_limitu / 3) { info[0] = .3; info[1] = (float)factor_g / originalGap; ret_val = -1; }
        else if (originalGap <= mid_limitu) { info[0] = .5; info[1] = 2.5; ret_val = 3; }
        else { info[0] = 1; info[1] = 1; info[2] = 1; ret_val = 1; }
    }
    return ret_val;
}

static vector<string> read_lines(const string &path, bool *ok) {
    vector<string> out;
    FILE *f = fopen(path.c_str(), "r");
    *ok = f != nullptr;
    if (!f) return out;
    char buf[MAX_REC_LEN];
    while (fgets(buf, MAX_REC_LEN, f) != NULL) out.emplace_back(buf);
    fclose(f);
    return out;
}

static vector<PartialRec> parse_partial_lines(const vector<string> &lines) {
    vector<PartialRec> out;
    for (const string &l : lines) {
        vector<char> b(l.begin(), l.end()); b.push_back('\0');
        char *sv = nullptr;
        PartialRec r;
        char *t = strtok_r(b.data(), "\t", &sv); r.seq = t ? t : "";
        t = strtok_r(NULL, "\t", &sv); r.clipped_index = t ? atoi(t) : 0;
        t = strtok_r(NULL, "\t", &sv); r.match = t ? atoi(t) : 0;
        t = strtok_r(NULL, "\t", &sv); r.pos = t ? atoi(t) : 0;
        strtok_r(NULL, "\t", &sv);
        t = strtok_r(NULL, "\t", &sv); r.ref_pos = t ? atoi(t) : 0;
        t = strtok_r(NULL, "\t", &sv); r.qual = t ? t : "";
        out.push_back(r);
    }
    return out;
}

struct GapOut { int gapNo, contigNo; long gapStart; int gapLength, gapStringLength; string str; };

// FillGaps.cpp:456-649 + writeGapLoad :313-334: which worker process fills which gaps.  tot <= T: one gap each.  Else
// `per` = ceil(tot/T) in float arithmetic; gaps of <= gapthresh bp go round the processes in turn; then the processes
// are ordered by how many more gaps they may take (std::sort, descending, as :603) and the long gaps either go one to
// each in that order (no more long gaps than processes) or fill each process up to `per` in that order.  Every list is
// sorted ascending before it is written.
static vector<vector<int>> deal_gaps_to_processes(const vector<int> &glen, int T, int gapthresh) {
    vector<vector<int>> P;
    int tot = (int)glen.size();
    if (T < 1) T = 1;
    if (tot <= T) { for (int i = 0; i < tot; i++) P.push_back(vector<int>(1, i)); return P; }
    float t_f = (float)(tot * 1.0 / T);
    int per = (int)t_f; if (t_f - (float)per > 0) per++;
    P.assign((size_t)T, vector<int>());
    vector<int> shortg, longg;
    for (int g = 0; g < tot; g++) { if (glen[(size_t)g] > gapthresh) longg.push_back(g); else shortg.push_back(g); }
    { size_t k = 0; while (k < shortg.size()) for (int i = 0; i < T && k < shortg.size(); i++) P[(size_t)i].push_back(shortg[k++]); }
    vector<vector<int>> loadrem((size_t)T, vector<int>(2, 0));
    for (int i = 0; i < T; i++) { loadrem[(size_t)i][0] = i; loadrem[(size_t)i][1] = per - (int)P[(size_t)i].size(); }
    std::sort(loadrem.begin(), loadrem.end(), [](const vector<int> &v1, const vector<int> &v2) { return v1[1] > v2[1]; });
    size_t k = 0;
    if ((int)longg.size() <= T) { for (int i = 0; i < T && k < longg.size(); i++) P[(size_t)loadrem[(size_t)i][0]].push_back(longg[k++]); }
    else for (int i = 0; i < T && k < longg.size(); i++) for (int j = 0; j < loadrem[(size_t)i][1] && k < longg.size(); j++) P[(size_t)loadrem[(size_t)i][0]].push_back(longg[k++]);
    for (auto &p : P) std::sort(p.begin(), p.end());
    return P;
}

// Per-gap driver, Figbird.cpp:7219-7466.  `mine[g]` says whether this "thread" owns gap g.
static bool run_gaps(const vector<char> &mine, vector<GapOut> &outs, FILE *draw) {
    bool ok;
    vector<string> gi = read_lines(A.tmp + "gapInfo.txt", &ok);
    if (!ok) { fprintf(stderr, "oracle: can't open gapInfo.txt\n"); return false; }
    vector<string> st2 = read_lines(A.tmp + "stat2.txt", &ok);
    if (!ok) { fprintf(stderr, "oracle: can't open stat2.txt\n"); return false; }
    size_t tot_gaps = gi.size();
    gaptofill.assign(tot_gaps, 0);
    drawf = draw;
    int r_count1 = 0, r_count2 = 0;
    for (size_t gapNo = 0; gapNo < tot_gaps && gapNo < st2.size(); gapNo++) {
        if (!(gapNo < mine.size() && mine[gapNo])) { gaptofill[gapNo] = -1; continue; }
        int fillflag = 1;
        left_maxDistance = A.D; right_maxDistance = A.D;
        int gapContigNo, gapLength; long gapStart;
        {
            vector<char> b(gi[gapNo].begin(), gi[gapNo].end()); b.push_back('\0');
            char *sv = nullptr;
            gapContigNo = atoi(strtok_r(b.data(), "\t", &sv));
            gapStart = atol(strtok_r(NULL, "\t", &sv));
            gapLength = atoi(strtok_r(NULL, "\t\n", &sv));
        }
        int ms[3] = {0, 0, 0};
        {
            vector<char> b(st2[gapNo].begin(), st2[gapNo].end()); b.push_back('\0');
            char *sv = nullptr;
            char *t = strtok_r(b.data(), "\t", &sv); ms[0] = t ? atoi(t) : 0;
            t = strtok_r(NULL, "\t", &sv); ms[1] = t ? atoi(t) : 0;
            t = strtok_r(NULL, "\t", &sv); ms[2] = t ? atoi(t) : 0;
        }
        string gname = A.gapsDir + "gaps_" + std::to_string(gapNo) + ".sam";
        string pname = A.gapsDir + "partial_gaps_" + std::to_string(gapNo) + ".sam";
        vector<string> ul, pl;
        if (A.unmapped == 1) {
            ul = read_lines(gname, &ok);
            r_count1 = (int)(ul.size() / 2);                // findcount_file(..,0)
            if (r_count1 > unmapped_limit) {
                printf("Gap = %zu\tReads = %d\n", gapNo, r_count1);
                r_count1 = unmapped_limit; fillflag = -1;
            }
        }
        pl = read_lines(pname, &ok);
        if (!ok) { fprintf(stderr, "oracle: missing %s (reference would crash)\n", pname.c_str()); return false; }
        vector<PartialRec> prec = parse_partial_lines(pl);
        if (A.partial_flag == 1) r_count2 = (int)std::min(pl.size(), (size_t)partial_limit + 1);   // findcount_file(..,1)
        GF gf;
        gf.contig = &SC.seq[gapContigNo]; gf.contigLen = (long)SC.seq[gapContigNo].size();
        gf.prec = &prec; gf.ulines = &ul;
        factor_g = 3 * A.partial_len;
        float info[3] = {0, 0, 0};
        int allocation_factor = findFrac(gapLength, info, 2 * A.partial_len, A.unm_limit);
        if (allocation_factor == -1) alloc_arg = factor_g * 3; else alloc_arg = gapLength * allocation_factor;
        gf.allocate(alloc_arg, r_count1, r_count2, A.read_length, ms[0], ms[1], ms[2], A.neg_lap, 2 * A.partial_len,
                    A.unm_limit, (int)info[2], info[0], info[1]);
        gf.gap_no = (int)gapNo; gf.gapStart = gapStart; gf.contigNo = gapContigNo; gf.originalGap = gapLength;
        gf.fillGap((int)gapNo, fillflag);
        GapOut o;
        o.gapNo = (int)gapNo; o.contigNo = gapContigNo; o.gapStart = gapStart; o.gapLength = gapLength;
        int len = gf.gapLength;
        o.str = gf.concensus.substr(0, std::min((size_t)std::max(len, 0), gf.concensus.size()));
        o.str.resize(std::max(len, 0), '\0');
        size_t z = o.str.find('\0');
        if (z != string::npos) o.str.resize(z);             // fprintf("%s") stops at the terminator
        o.gapStringLength = len;
        outs.push_back(o);
    }
    return true;
}

static void write_gapout(const string &path, const vector<GapOut> &outs) {
    FILE *f = fopen(path.c_str(), "w");
    for (const GapOut &o : outs)
        fprintf(f, "%d\t%d\t%ld\t%d\t%d\t%s\n", o.gapNo, o.contigNo, o.gapStart, o.gapLength, o.gapStringLength, o.str.c_str());
    fclose(f);
}

// Scaffold rebuild + Ncount, FillGaps.cpp:708-926.  `gtf` is consumed (decremented) like the reference's array.
static void rebuild_scaffold(const vector<GapOut> &outs_sorted, vector<int> gtf) {
    FILE *out = fopen((A.tmp + "filledContigs.fa").c_str(), "w");
    FILE *nf = fopen((A.tmp + "Ncount.txt").c_str(), "w");
    int nStart = 0, nCount = 0, gap_count = -1;
    int prevNcount = 0, newNcount = 0;
    size_t next_out = 0;
    string gapString;                                        // persists across gaps (stale when length 0, :870)
    int gapStringLength = 0;
    for (size_t i = 0; i < SC.seq.size(); i++) {
        const string &ctgs = SC.seq[i];
        string contig;
        fprintf(out, ">%s\n", i < SC.names.size() ? SC.names[i].c_str() : "");
        long n = (long)ctgs.size();
        for (long j = 0; j < n; j++) {
            bool condition = (ctgs[j] == 'N' || ctgs[j] == 'n');
            if (condition) {
                if (nStart == 0) { nStart = 1; nCount = 1; gap_count++; }
                else nCount++;
            }
            if (!condition || (condition && j == n - 1)) {
                if (nStart == 1) {
                    prevNcount += nCount;
                    if (next_out < outs_sorted.size()) {
                        const GapOut &o = outs_sorted[next_out++];
                        gapStringLength = o.gapStringLength;
                        if (gapStringLength > 0) gapString = o.str;
                    }
                    for (char c : gapString) if (c == 'N') newNcount++;
                    fputs(contig.c_str(), out);
                    if (gapStringLength > 0) fputs(gapString.c_str(), out);
                    contig.clear();
                    nStart = 0;
                }
                if (gap_count >= 0 && gap_count < (int)gtf.size() && gtf[gap_count] > 0) gtf[gap_count]--;
                else contig.push_back(ctgs[j]);
            }
        }
        fprintf(out, "%s\n", contig.c_str());
    }
    int fillmore = (newNcount == 0) ? 0 : 1;                // FillGaps.cpp:920-922
    fprintf(nf, "%d", fillmore);
    fclose(out);
    fclose(nf);
}

static int oracle_main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: figbird_oracle figbird|fillgaps <args>\n"); return 2; }
    string mode = argv[1];
    init_char_codes();
    lm_jit_init();
    const char *tr = getenv("FIG_ORACLE_TRACE");
    if (tr) { g_trace = fopen(tr, "w"); const char *lv = getenv("FIG_ORACLE_TRACE_LEVEL"); g_trace_level = lv ? atoi(lv) : 1;
              if (g_trace_level >= 5) { g_trace_det = 1; g_trace_level -= 4; } }        // 5..8: levels 1..4 plus the DET lines
    int thread_id = 0, totalgapstofill = 0, num_threads = 1;
    if (mode == "figbird") {
        if (argc < 17) { fprintf(stderr, "figbird mode needs 15-16 args\n"); return 2; }
        char **a = argv + 1;
        A.contigFile = a[1]; A.D = atoi(a[2]); A.read_length = atoi(a[3]); A.script_itr = atoi(a[4]);
        A.partial_flag = atoi(a[5]); A.unmapped = atoi(a[6]); thread_id = atoi(a[7]); totalgapstofill = atoi(a[8]);
        A.mapFile = a[9]; A.tmp = a[10]; A.gapsDir = a[11]; A.neg_lap = atoi(a[12]); A.partial_len = atoi(a[13]);
        A.unm_limit = atoi(a[14]); A.setinputmean = atoi(a[15]);
        if (A.setinputmean == 1 && argc > 17) A.isz = atoi(a[16]);
    } else if (mode == "fillgaps") {
        if (argc < 17) { fprintf(stderr, "fillgaps mode needs 15 args\n"); return 2; }
        char **a = argv + 1;
        A.contigFile = a[1]; A.D = atoi(a[2]); A.read_length = atoi(a[3]); A.script_itr = atoi(a[4]);
        A.partial_flag = atoi(a[5]); A.unmapped = atoi(a[6]); num_threads = atoi(a[7]);
        A.mapFile = a[8]; A.tmp = a[9]; A.gapsDir = a[10]; A.neg_lap = atoi(a[11]); A.partial_len = atoi(a[12]);
        A.setinputmean = atoi(a[14]); A.isz = atoi(a[15]);
        A.unm_limit = 400;                                   // gapthresh, FillGaps.cpp:22,119
    } else { fprintf(stderr, "unknown mode %s\n", mode.c_str()); return 2; }
    if (!load_scaffolds(A.contigFile.c_str(), SC)) { printf("Can't open contig file\n"); return 1; }
    if (!build_model()) return 1;
    if (g_trace) {
        fprintf(g_trace, "MODEL\t%d\t%d\t%d\t%a\t%a\t%a\n", M.gapProbCutOff, M.insertThresholdMin, M.insertThresholdMax,
                M.insertSizeMean, M.leftSD, M.rightSD);
    }
    bool ok;
    vector<string> gi = read_lines(A.tmp + "gapInfo.txt", &ok);
    size_t tot_gaps = gi.size();
    vector<char> mine(tot_gaps, 0);
    if (mode == "figbird") {
        // gaploads.txt line <thread_id>: tab-separated gap ids (Figbird.cpp:7277-7317)
        vector<string> gl = read_lines(A.tmp + "gaploads.txt", &ok);
        if (ok && (size_t)thread_id < gl.size()) {
            vector<char> b(gl[thread_id].begin(), gl[thread_id].end()); b.push_back('\0');
            char *sv = nullptr; int cnt = 0;
            for (char *t = strtok_r(b.data(), "\t\n ", &sv); t && cnt < totalgapstofill; t = strtok_r(NULL, "\t\n ", &sv), cnt++) {
                int id = atoi(t);
                if (id >= 0 && (size_t)id < tot_gaps) mine[id] = 1;
            }
        }
    } else for (size_t i = 0; i < tot_gaps; i++) mine[i] = 1;

    string sfx = mode == "figbird" ? std::to_string(thread_id) : string();
    FILE *draw = fopen((A.tmp + "draw" + sfx + ".txt").c_str(), "w");
    vector<GapOut> outs;
    vector<int> gtf_merged;
    if (mode == "fillgaps" && tot_gaps > 0) {
        // FillGaps.cpp:456-679: the gaps are dealt to `num_threads` worker processes, each a fresh `Figbird.cpp main` over its
        // line of gaploads.txt (ascending gap ids); their draw files are concatenated in process order (mergeFiles :222-260),
        // their gapout lines merged by gap number (readgapouts :140-219), their gaptofill arrays by ownership (readGtf).
        vector<int> glen(tot_gaps, 0);
        for (size_t g = 0; g < tot_gaps; g++) {
            vector<char> b2(gi[g].begin(), gi[g].end()); b2.push_back('\0');
            char *sv = nullptr; strtok_r(b2.data(), "\t", &sv); strtok_r(NULL, "\t", &sv);
            char *t = strtok_r(NULL, "\t\n", &sv); glen[g] = t ? atoi(t) : 0;
        }
        vector<vector<int>> procs = deal_gaps_to_processes(glen, num_threads, 400);
        { FILE *f = fopen((A.tmp + "gaploads.txt").c_str(), "w");            // writeGapLoad :313-334
          if (f) { for (auto &pr : procs) { for (int g : pr) fprintf(f, "%d\t", g); fprintf(f, "\n"); } fclose(f); } }
        gtf_merged.assign(tot_gaps, 0);
        for (auto &pr : procs) {
            // globals of a fresh process (Figbird.cpp:99-147 are zero-initialised)
            factor_g = covergae_threshold1 = covergae_threshold2 = partial_threshold = overlap_threshold = 0;
            match_count_discont = clip_thresh = num_itr = alloc_arg = step2match = 0;
            std::fill(mine.begin(), mine.end(), 0);
            for (int g : pr) mine[(size_t)g] = 1;
            vector<GapOut> o1;
            if (!run_gaps(mine, o1, draw)) return 1;
            for (auto &o : o1) outs.push_back(o);
            for (int g : pr) if (gaptofill[(size_t)g] != -1) gtf_merged[(size_t)g] = gaptofill[(size_t)g];
        }
        std::sort(outs.begin(), outs.end(), [](const GapOut &x, const GapOut &y) { return x.gapNo < y.gapNo; });
    } else if (!run_gaps(mine, outs, draw)) return 1;
    if (draw) fclose(draw);
    write_gapout(A.tmp + "gapout" + sfx + ".txt", outs);
    if (mode == "figbird") {
        FILE *f = fopen((A.tmp + "gaptofill" + sfx + ".txt").c_str(), "w");
        for (size_t i = 0; i < tot_gaps; i++) fprintf(f, "%d\n", gaptofill[i]);
        fclose(f);
    } else {
        vector<int> gtf(tot_gaps, 0);                        // readGtf: -1 entries leave 0 (FillGaps.cpp:288-297)
        if (!gtf_merged.empty()) gtf = gtf_merged;
        else for (size_t i = 0; i < tot_gaps; i++) if (gaptofill[i] != -1) gtf[i] = gaptofill[i];
        rebuild_scaffold(outs, gtf);
    }
    if (g_trace) { fprintf(g_trace, "STATS\t%ld\t%.17g\n", g_place_calls, g_flops); fclose(g_trace); }
    const char *st = getenv("FIG_ORACLE_STATS");
    if (st) { FILE *f = fopen(st, "w"); if (f) { fprintf(f, "%ld %.17g\n", g_place_calls, g_flops); fclose(f); } }
    return 0;
}
