// Host check of goliath_amd/csrc/gol_lbs_math.h: every derivative the skeleton backward uses against central differences of
// the forward function it belongs to, at random arguments, in double.  Prints one line per function; the exit status is the
// number of functions whose worst |difference| exceeds 1e-7 (step 1e-6, values of order 1: truncation error ~1e-10).
// Built and run by tests/test_lbs_host.py.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <vector>
#include "../goliath_amd/csrc/gol_lbs_math.h"
using namespace gol_lbs;
typedef std::vector<double> vec;
static int failures = 0;
double rnd(){return (rand()/(double)RAND_MAX-0.5)*2;}
// check analytic grad of sum(cot*f(x)) vs central differences
void check(const char*name, int n, int m, std::function<vec(const vec&)> f, std::function<vec(const vec&,const vec&)> bwd){
  vec x(n),c(m); for(auto&v:x)v=rnd(); for(auto&v:c)v=rnd();
  vec g=bwd(x,c); double worst=0;
  for(int i=0;i<n;i++){ vec a=x,b=x; double h=1e-6; a[i]+=h;b[i]-=h; vec fa=f(a),fb=f(b); double d=0; for(int k=0;k<m;k++)d+=c[k]*(fa[k]-fb[k])/(2*h); worst=fmax(worst,fabs(d-g[i])); }
  printf("%-20s worst |fd - analytic| = %.3e\n",name,worst);
  if(!(worst<1e-7)) ++failures;
}
State S(const double*p){return {{p[0],p[1],p[2]},{p[3],p[4],p[5],p[6]},p[7]};}
void put(vec&o,const State&s){o.insert(o.end(),{s.t.x,s.t.y,s.t.z,s.q.x,s.q.y,s.q.z,s.q.w,s.s});}
int main(){
  check("qmul",8,4,[](const vec&x){Q4 r=qmul({x[0],x[1],x[2],x[3]},{x[4],x[5],x[6],x[7]});return vec{r.x,r.y,r.z,r.w};},
    [](const vec&x,const vec&c){Q4 g={c[0],c[1],c[2],c[3]};Q4 a=qmul_bwd_q({x[4],x[5],x[6],x[7]},g),b=qmul_bwd_r({x[0],x[1],x[2],x[3]},g);return vec{a.x,a.y,a.z,a.w,b.x,b.y,b.z,b.w};});
  check("qrot",7,3,[](const vec&x){D3 r=qrot({x[0],x[1],x[2],x[3]},{x[4],x[5],x[6]});return vec{r.x,r.y,r.z};},
    [](const vec&x,const vec&c){Q4 gq;D3 gv;qrot_bwd({x[0],x[1],x[2],x[3]},{x[4],x[5],x[6]},{c[0],c[1],c[2]},gq,gv);return vec{gq.x,gq.y,gq.z,gq.w,gv.x,gv.y,gv.z};});
  check("from_xyz",3,4,[](const vec&x){Q4 r=from_xyz(half_trig({x[0],x[1],x[2]}));return vec{r.x,r.y,r.z,r.w};},
    [](const vec&x,const vec&c){D3 g=from_xyz_bwd(half_trig({x[0],x[1],x[2]}),{c[0],c[1],c[2],c[3]});return vec{g.x,g.y,g.z};});
  // compose: x = parent state (8) + lt(3) + lr(4) + ls(1)
  check("compose",16,8,[](const vec&x){State r=compose(S(&x[0]),{x[8],x[9],x[10]},{x[11],x[12],x[13],x[14]},x[15]);vec o;put(o,r);return o;},
    [](const vec&x,const vec&c){State gp;D3 glt;Q4 glr;double gls;compose_bwd(S(&x[0]),{x[8],x[9],x[10]},{x[11],x[12],x[13],x[14]},x[15],S(&c[0]),gp,glt,glr,gls);vec o;put(o,gp);o.insert(o.end(),{glt.x,glt.y,glt.z,glr.x,glr.y,glr.z,glr.w,gls});return o;});
  vec bi(8);for(auto&v:bi)v=rnd();
  check("state_to_matrix",8,12,[&](const vec&x){double m[12];state_to_matrix(S(&x[0]),S(&bi[0]),m);return vec(m,m+12);},
    [&](const vec&x,const vec&c){State g=state_to_matrix_bwd(S(&x[0]),S(&bi[0]),&c[0]);vec o;put(o,g);return o;});
  vec pre(4),off(3);for(auto&v:pre)v=rnd();for(auto&v:off)v=rnd();
  check("local_transform",7,8,[&](const vec&x){D3 lt;Q4 lr;double ls;local_transform(&x[0],{off[0],off[1],off[2]},{pre[0],pre[1],pre[2],pre[3]},lt,lr,ls);return vec{lt.x,lt.y,lt.z,lr.x,lr.y,lr.z,lr.w,ls};},
    [&](const vec&x,const vec&c){double gp[7];local_transform_bwd(&x[0],{pre[0],pre[1],pre[2],pre[3]},exp2(x[6]),{c[0],c[1],c[2]},{c[3],c[4],c[5],c[6]},c[7],gp);return vec(gp,gp+7);});
  return failures;
}
